/*
 * libdis_hip.so -- C ABI of the MI355X (gfx950) DIS-SF / DIS-MF training-step kernels.
 *
 * This is the drop-in boundary.  The reference's only native seam is the
 * pybind module pair `ext_cpu` / `ext_cuda` of connecting_the_dots' torchext, bound at
 *   /root/reference/model/ext_functions.py:32-39   (import by bare name from CTD_DIR/torchext)
 *   /root/reference/model/ext_functions.py:124,126 (photometric_loss_forward)
 *   /root/reference/model/ext_functions.py:137,139 (photometric_loss_backward)
 * `dis_photometric_fwd/bwd` replace exactly those two entry points.  Every other function below
 * replaces a group of ATen/cuDNN operator calls inside model/networks.py and
 * model/multi_frame_networks.py (cited per function); the reference has no native code for them.
 *
 * Conventions
 *  - plain C symbols, raw DEVICE pointers, sizes as int, no torch types.
 *  - the caller owns every buffer (inputs, outputs, workspaces); the library never allocates,
 *    frees or synchronises.  All calls are asynchronous on `stream` (a hipStream_t passed as
 *    void*) and graph-capturable.  Process-wide state is limited to: (1) the operand split of the
 *    `*_bf16x3*` entry points (dis_set_conv_split / DIS_CONV_SPLIT: the entry points keep their
 *    round-1 names, the arithmetic they run is two-term fp16 by default, three-term bf16 on request
 *    - dis_get_conv_split() tells which); (2) one-time hipFuncSetAttribute flags per kernel;
 *    (3) the diagnostic tag of dis_last_kernel().  None of it is per-call data: calls from several
 *    host threads on different streams are safe as long as no thread changes the split meanwhile.
 *  - return value: 0 on success, DIS_ERR_* (<0) on a rejected argument, or the positive hipError_t
 *    of a failed launch.  Nothing throws across the boundary.
 *  - "planar" tensors are (N,C,H,W) contiguous fp32 (the reference layout, used for the 1-3 channel
 *    images/disparities/flows of the module API).  "nhwc" tensors are (N,H,W,C) contiguous fp32 and
 *    are used for every feature map inside the networks (one pixel of 32 channels = one 128-B line).
 *  - reductions to a scalar accumulate in fp64 in a caller-provided, ZEROED `double` workspace.
 */
#ifndef DIS_HIP_H
#define DIS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DIS_OK 0
#define DIS_ERR_BAD_SHAPE (-1)
#define DIS_ERR_UNSUPPORTED (-2)
#define DIS_ERR_NULL (-3)

#define DIS_ACT_NONE 0
#define DIS_ACT_SELU 1
#define DIS_ACT_RELU 2
/* OR-ed into the `act` argument of dis_conv2d_fwd: y = act(y_previous + conv(x) + bias) (sum of convolutions over
 * several input tensors = a convolution over their channel concatenation; accumulation of input gradients). */
#define DIS_CONV_ACCUM 0x100

/* ABI version of this header; bumped on any signature change. */
int dis_abi_version(void);

/* ---------------------------------------------------------------- per-pixel operators ------- */

/* Local contrast normalisation, reference model/networks.py:663-689 (LCN.tforward).
 * x, out_lcn, out_std: (n,1,h,w).  reflect pad `radius`, (2r+1)^2 box sums. */
int dis_lcn_fwd(const float* x, float* out_lcn, float* out_std, int n, int h, int w, int radius, float eps,
                void* stream);

/* Photometric window loss, replaces ext_{cpu,cuda}.photometric_loss_forward
 * (reference model/ext_functions.py:124,126; arithmetic per :156-183).
 * es, ta: (n,c,h,w); out: (n,1,h,w).  type: 0 mse, 1 sad, 2 census_mse, 3 census_sad. block odd <= 15. */
int dis_photometric_fwd(const float* es, const float* ta, float* out, int n, int c, int h, int w, int block,
                        int type, float eps, void* stream);
/* replaces photometric_loss_backward (reference model/ext_functions.py:137,139): gradient wrt `es` only. */
int dis_photometric_bwd(const float* es, const float* ta, const float* grad_out, float* grad_es, int n, int c,
                        int h, int w, int block, int type, float eps, void* stream);
/* The census forms (type 2 / 3, 9 x 9 window, one channel) for S <= 4 estimates against ONE target in a single launch: DIS-SF
 * compares its four output scales with the same LCN image (reference model/single_frame_worker.py:110-118), and the soft sign of the
 * target differences is the same for all of them.  es, out, grad_out, grad_es: (s, n, 1, h, w) stacked; ta (n, 1, h, w).
 * Equal to s calls of dis_photometric_fwd / _bwd to rounding.  Other types / windows: DIS_ERR_UNSUPPORTED. */
int dis_photometric_fwd_multi(const float* es, const float* ta, float* out, int s, int n, int h, int w, int block, int type,
                              float eps, void* stream);
int dis_photometric_bwd_multi(const float* es, const float* ta, const float* grad_out, float* grad_es, int s, int n, int h,
                              int w, int block, int type, float eps, void* stream);


/* Pattern projection of RectifiedPatternSimilarityLoss, reference model/networks.py:358-367:
 * proj[n,y,x] = bilinear(pattern, x - disp[n,y,x], y), align_corners=True, padding 'border'.
 * pattern: (1,1,h,w) shared by all n.  disp, proj: (n,1,h,w). */
int dis_pattern_warp_fwd(const float* pattern, const float* disp, float* proj, int n, int h, int w, void* stream);
/* grad_disp = -grad_proj * d(sample)/dx   (the only path by which the photometric loss reaches the net). */
int dis_pattern_warp_bwd(const float* pattern, const float* disp, const float* grad_proj, float* grad_disp, int n,
                         int h, int w, void* stream);

/* val = sum(w*x)/sum(w) (reference model/networks.py:374), or mean(|x-y|) style reductions.
 * acc: 2 zeroed doubles {sum(w*x), sum(w)}; out: 1 float.  w may be NULL (=> plain mean over count). */
int dis_weighted_mean_fwd(const float* x, const float* w, double* acc, float* out, long count, void* stream);
/* grad_x = gscale[0] * w / sum(w)  (acc as left by the forward). */
int dis_weighted_mean_bwd(const float* w, const double* acc, const float* gscale, float* grad_x, long count,
                          void* stream);

/* mean(|a-b|)  (warm-up / pseudo-GT L1, reference model/multi_frame_worker.py:164, single_frame_worker.py:154) */
int dis_l1_mean_fwd(const float* a, const float* b, double* acc, float* out, long count, void* stream);
/* grad_a = gscale[0] * sign(a-b) / count */
int dis_l1_mean_bwd(const float* a, const float* b, const float* gscale, float* grad_a, long count, void* stream);

/* Real-data warm-up term (reference model/multi_frame_worker.py:168-173, single_frame_worker.py:158-163):
 * valid = sgm_disp > thresh (30); out = sum(|out_disp - sgm_disp + noise| * valid) / sum(valid).  noise is the caller's
 * 1.5 * N(0,1) draw (the reference draws it on the host generator and copies it over).  acc: 2 zeroed doubles. */
int dis_sgm_l1_fwd(const float* out_disp, const float* sgm_disp, const float* noise, float thresh, double* acc,
                   float* out, long count, void* stream);
int dis_sgm_l1_bwd(const float* out_disp, const float* sgm_disp, const float* noise, float thresh, const double* acc,
                   const float* gscale, float* grad_out_disp, long count, void* stream);

/* Masked multi-scale pseudo-GT term (DIS-FTSF on a target with holes, e.g. <track>/raycast_<disp>.npz): n = 1 .. 4 estimates against
 * ONE target, all float32, contiguous, seen as (planes, h, w); est_host / grad_host: HOST arrays of n device pointers (copied into
 * the kernel arguments by value: a captured call holds them).  erode = r in 0 .. 3.
 *   valid(p, y, x)  target > 0 at every pixel of the (2r+1)^2 window around (y, x) that lies inside the image, in plane p (pixels
 *                   outside the image do not invalidate; NaN is not > 0: a hole)
 *   out[s]          (float)(sum over valid of (double)|est_s - target| / (double)N), N = valid pixels of the whole call; 0 when N = 0
 *   grad_s[i]       valid_i ? sign(est_s[i] - target[i]) * (gscale[s] / (float)N) : 0   (sign(0) = 0; all 0 when N = 0)
 * Masking is a select: a non-finite estimate or target under a hole contributes nothing.  acc: dis_masked_l1_multi_acc_doubles()
 * doubles of scratch (no zeroing), kept for the backward, which reads N from it: record 0 = {sum_0 .. sum_3, N}, behind it one such
 * record per workgroup, added in index order by a second launch - no atomics, the grid depends on the shape alone, so out and grad
 * have the same bits on every run.  Forward: two launches, backward: one, for any n; nothing is read back to the host.
 * gscale: n device floats.  tests/masked_l1_ref.py restates the arithmetic in numpy. */
long dis_masked_l1_multi_acc_doubles(void);
int dis_masked_l1_multi_fwd(const float* const* est_host, int n, const float* target, int erode, double* acc, float* out, int planes,
                            int h, int w, void* stream);
int dis_masked_l1_multi_bwd(const float* const* est_host, int n, const float* target, int erode, const double* acc,
                            const float* gscale, float* const* grad_host, int planes, int h, int w, void* stream);

/* DisparitySmoothLoss, reference model/networks.py:411-431 with SobelFilter(ksize=5) :693-731.
 * disp, amb: (n,1,h,w).  acc: 1 zeroed double; out: 1 float = mean over (n,2,h,w). */
int dis_smooth_loss_fwd(const float* disp, const float* amb, double* acc, float* out, int n, int h, int w,
                        void* stream);
/* grad_disp is OVERWRITTEN (the scatter through the 5x5 taps is done as a gather, no atomics).
 * workspace: 2*n*h*w floats. */
int dis_smooth_loss_bwd(const float* disp, const float* amb, const float* gscale, float* grad_disp,
                        float* workspace, int n, int h, int w, void* stream);

/* DispToDepth, reference model/networks.py:311-319: depth = bf / (relu(disp) + 1e-12) */
int dis_disp_to_depth_fwd(const float* disp, float* depth, float bf, long count, void* stream);
int dis_disp_to_depth_bwd(const float* disp, const float* grad_depth, float* grad_disp, float bf, long count,
                          void* stream);

/* One direction of the flow-consistency (geometric) loss:
 *   multi-frame  reference model/networks.py:564-601  (primary_depth1 != NULL: adds the rf mask)
 *   single-frame reference model/networks.py:619-655  (clamp > 0: diff clamped to [0,clamp])
 * depth0, depth1, amb0, amb1, primary_depth1: (bs,1,h,w); flow0, flow1: (bs,2,h,w) pixel units;
 * R0,R1: (bs,3,3); t0,t1: (bs,3) device pointers; K: 9 floats, Kinv: 9 floats (host values, by pointer to host).
 * mask_out: (bs,1,h,w) {0,1} loss mask (saved for backward); acc: dis_geo_loss_acc_doubles() doubles of scratch (no zeroing):
 * acc[0], acc[1] = {sum(diff*mask), sum(mask)} after the call (dis_geo_loss_bwd reads them), behind them the per-block partial
 * sums they are formed from in a fixed order; out: 1 float = acc0/(acc1+1e-8). */
long dis_geo_loss_acc_doubles(void);
int dis_geo_loss_fwd(const float* depth0, const float* depth1, const float* flow0, const float* flow1,
                     const float* amb0, const float* amb1, const float* primary_depth1, const float* R0,
                     const float* t0, const float* R1, const float* t1, const float* K_host,
                     const float* Kinv_host, float clamp, float* mask_out, double* acc, float* out, int bs, int h,
                     int w, void* stream);
/* grad_depth0 (bs,1,h,w) is WRITTEN (+=); grad_depth1 (bs,1,h,w) is scatter-added (atomics).  Both must be
 * valid accumulators (zeroed or holding earlier contributions). */
int dis_geo_loss_bwd(const float* depth0, const float* depth1, const float* flow0, const float* R0,
                     const float* t0, const float* R1, const float* t1, const float* K_host,
                     const float* Kinv_host, float clamp, const float* mask, const double* acc,
                     const float* gscale, float* grad_depth0, float* grad_depth1, int bs, int h, int w,
                     void* stream);

/* Round 5: ALL directional terms of a step - tl (tl - 1) = 12 (reference model/multi_frame_worker.py:139-158, single_frame_worker.py
 * :126-149; model/networks.py:554-661) - in one forward and one backward launch.  terms: HOST array of nterms <= 16 tables of DEVICE
 * pointers, argument for argument those of dis_geo_loss_fwd / _bwd (pdepth1 may be NULL: no primary-depth mask; flow1 / amb0 / amb1
 * are not read by the backward; gdepth0 / gdepth1 not by the forward).  acc: dis_geo_loss_multi_acc_doubles(nterms) doubles (kept for
 * the backward); out (nterms) floats: the values of nterms single calls, bit for bit.  Backward: gscale (nterms) device floats;
 * both depth gradients are ADDED with float atomics into gdepth0 / gdepth1 (zeroed or pre-filled by the caller; terms may share
 * them): equal to the single calls to rounding. */
typedef struct DisGeoTerm {
  const float *depth0, *depth1, *flow0, *flow1, *amb0, *amb1, *pdepth1, *R0, *t0, *R1, *t1;
  float *mask, *gdepth0, *gdepth1;
} DisGeoTerm;
long dis_geo_loss_multi_acc_doubles(int nterms);
int dis_geo_loss_fwd_multi(const DisGeoTerm* terms, int nterms, const float* K_host, const float* Kinv_host, float clampv, double* acc,
                           float* out, int bs, int h, int w, void* stream);
int dis_geo_loss_bwd_multi(const DisGeoTerm* terms, int nterms, const float* K_host, const float* Kinv_host, float clampv,
                           const double* acc, const float* gscale, int bs, int h, int w, void* stream);

/* The two backward entry points above (the gradient of reference model/networks.py:564-601 / :619-655 wrt both depths; the terms of
 * model/multi_frame_worker.py:139-158, single_frame_worker.py:126-149) with sums that do not depend on the order of arrival: the
 * same inputs give the same bits on every call.  Per term the scattered depth1 addend -gs sigma w (gs uniform over the term, sigma =
 * mask x sign in {-1, 0, 1}, w a bilinear weight) is accumulated as -sigma rint(w 2^32) in a 64-bit integer cell per pixel, the
 * depth0 addend is stored; a second pass walks the terms of every distinct gradient plane in table order, adds
 * (double)v_k + (double)gs_k ((double)S_k 2^-32), rounds to fp32 once and ADDS the result to the plane (plain read-modify-write:
 * zeroed or pre-filled by the caller, like the atomic forms; the single-term grad_depth0 is the atomic form's bit for bit).
 * Gradient planes are told apart by pointer: two planes are the same pointer or do not overlap.
 * workspace: dis_geo_loss_bwd_det_workspace(nterms, bs, h, w) bytes (-1: nterms outside 1..16 or a non-positive extent; 1 term for
 * dis_geo_loss_bwd_det), 8-byte aligned, no zeroing - the entry point clears what it sums into, on `stream`, without
 * synchronising or allocating (capturable). */
long dis_geo_loss_bwd_det_workspace(int nterms, int bs, int h, int w);
int dis_geo_loss_bwd_det(const float* depth0, const float* depth1, const float* flow0, const float* R0,
                         const float* t0, const float* R1, const float* t1, const float* K_host,
                         const float* Kinv_host, float clamp, const float* mask, const double* acc,
                         const float* gscale, float* grad_depth0, float* grad_depth1, int bs, int h, int w,
                         void* workspace, void* stream);
int dis_geo_loss_bwd_multi_det(const DisGeoTerm* terms, int nterms, const float* K_host, const float* Kinv_host, float clampv,
                               const double* acc, const float* gscale, int bs, int h, int w, void* workspace, void* stream);

/* ---------------------------------------------------------------- layout / resize / warp ---- */

/* Pack up to 4 planar single-channel sources (n,1,h,w) into nhwc C=4 (NULL source => zeros).
 * Used for the FuseNet stem input cat(ir(2), amb, d) (reference multi_frame_networks.py:217,273). */
int dis_pack4_nhwc(const float* s0, const float* s1, const float* s2, const float* s3, float* out, int n, int h,
                   int w, void* stream);
/* same with a per-source sample stride (floats), e.g. the two planes of an (n,2,h,w) tensor: stride 2*h*w */
int dis_pack4_nhwc_strided(const float* s0, long st0, const float* s1, long st1, const float* s2, long st2,
                           const float* s3, long st3, float* out, int n, int h, int w, void* stream);
/* planar (n,c,h,w) <-> nhwc (n,h,w,c) */
int dis_planar_to_nhwc(const float* x, float* y, int n, int c, int h, int w, void* stream);
int dis_nhwc_to_planar(const float* x, float* y, int n, int c, int h, int w, void* stream);

/* Bilinear resize (F.interpolate mode='bilinear'), reference multi_frame_networks.py:47,63,246,420,422
 * (align_corners=1) and networks.py:273-293 (align_corners=0).  nhwc, any c.
 * scale_x/scale_y multiply channel 0 / channel 1 of the result when c==2 && flow_scale!=0
 * (resize_flow_like, reference multi_frame_networks.py:64-65). */
int dis_resize_bilinear_nhwc_fwd(const float* x, float* y, int n, int hin, int win, int hout, int wout, int c,
                                 int align_corners, void* stream);
int dis_resize_bilinear_nhwc_bwd(const float* gy, float* gx /*zeroed*/, int n, int hin, int win, int hout, int wout,
                                 int c, int align_corners, void* stream);
int dis_resize_bilinear_planar_fwd(const float* x, float* y, int nc, int hin, int win, int hout, int wout,
                                   int align_corners, float scale0, float scale1, int c_for_scale, void* stream);
int dis_resize_bilinear_planar_bwd(const float* gy, float* gx, int nc, int hin, int win, int hout, int wout,
                                   int align_corners, void* stream);

/* gather_warped_feat for all targets, reference multi_frame_networks.py:347-360 + warp :83-99.
 * feat: (tl,bs,h,w,c) nhwc; flows: (tl*tl, bs, h, w, 2) nhwc, entry [i*tl+j] = flow_ij (diagonal unused).
 * out: (tl, bs, h, w, tl, c): slot 0 = own frame, slots 1.. = other frames in increasing index, warped. */
int dis_gather_warped_feat_fwd(const float* feat, const float* flows, float* out, int tl, int bs, int h, int w,
                               int c, void* stream);
/* grad_feat is OVERWRITTEN: own-frame slot by plain stores, then the warped slots scatter-add (float atomics). */
int dis_gather_warped_feat_bwd(const float* grad_out, const float* flows, float* grad_feat, int tl, int bs, int h,
                               int w, int c, void* stream);

/* Deterministic, atomic-free form of the same backward.  dis_gather_csr_build turns `flows` into a CSR index by
 * destination pixel (lists sorted by source row) once per step and resolution: csr = dis_gather_csr_workspace(...)
 * int32 words; every dis_gather_warped_feat_bwd_csr call with the same flows then gathers whole rows of grad_out with
 * plain loads (grad_feat OVERWRITTEN, bitwise reproducible).  `init` (optional, may alias grad_feat) is a second
 * gradient of `feat` (e.g. its residual branch) that is added in the same pass. */
long dis_gather_csr_workspace(int tl, int bs, int h, int w);
int dis_gather_csr_build(const float* flows, int* csr, int tl, int bs, int h, int w, void* stream);
int dis_gather_warped_feat_bwd_csr(const float* grad_out, const int* csr, const float* init, float* grad_feat, int tl,
                                   int bs, int h, int w, int c, void* stream);
/* Round 6 - dis_gather_warped_feat_bwd_csr when `feat` IS y = act(GroupNorm(x2) + residual) (a Block2D3D / ResNetBlock output,
 * reference model/multi_frame_networks.py:428-430, 540-542) and this launch completes the gradient wrt y: grad_feat receives
 * gres = g act'(y) (the pre-activation gradient = the residual gradient), ab_out (tl * bs, slots, 2, c) doubles - ZEROED by the caller,
 * slots = dis_conv2d_gnsums_slots() - the channel sums dis_gn_bwd_coef takes.  Replaces the dis_gn_bwd_res_sums pass over g, y, x2.
 * DIS_ERR_UNSUPPORTED: no tiled instance (the caller runs the two launches). */
int dis_gather_warped_feat_bwd_csr_gnres(const float* grad_out, const int* csr, const float* init, float* grad_feat, const float* y,
                                         const float* x2, double* ab_out, int slots, int act, int tl, int bs, int h, int w, int c,
                                         void* stream);

/* unproject + change_view_angle + gather_warped_xyz + forward/backward flow mask for every target,
 * reference multi_frame_networks.py:172-214,283-294.  No gradient.
 * depth_core: (tl,bs,h,w); R (tl,bs,3,3), t (tl,bs,3) device; Kinv_host 9 floats;
 * ray uses the pixel coordinates (u_step*x, v_step*y) (even full-res pixels for the core grid).
 * out: (tl, bs, h, w, tl, 4) = xyz + mask per slot. */
int dis_mf_geometry(const float* depth_core, const float* R, const float* t, const float* flows,
                    const float* Kinv_host, int u_step, int v_step, float* out, int tl, int bs, int h, int w,
                    void* stream);
/* quarter-resolution version: bilinear (align_corners) resize of `geom` and mask re-binarised with >0.5
 * (reference multi_frame_networks.py:393-394). */
int dis_mf_geometry_resize(const float* geom, float* out, int tl, int bs, int hin, int win, int hout, int wout,
                           void* stream);

/* ---------------------------------------------------------------- dense layers -------------- */

/* Repack OIHW weights (cout,cin_real,k,k) into the LDS fragment order of dis_conv2d_fwd.
 * mode 0 = forward: the packed conv has cin_pad >= cin_real input channels (extra ones get zero weights,
 *          e.g. the 1-channel ambient conv runs as a 4-channel conv on a zero-padded nhwc4 input).
 * mode 1 = stride-1 input gradient: spatially flipped, cin<->cout swapped (cin_pad must equal cin_real).
 * packed has k*k*cin_pad*cout floats. */
int dis_conv2d_pack_weights(const float* w_oihw, float* packed, int cout, int cin_real, int cin_pad, int k,
                            int mode, void* stream);

/* Implicit-GEMM convolution on the matrix cores (v_mfma_f32_16x16x4_f32: fp32 in, fp32 accumulate), nhwc.
 * Replaces ZeroPad2d + Conv2d (+SELU/ReLU) of reference multi_frame_networks.py:159-164,330-345,514-542
 * and Conv2d of networks.py:222-234.
 * x: (n,hin,win,cin); y: (n,hout,wout,cout), hout = (hin + 2*pad - k)/stride + 1.
 * bias may be NULL.  act: DIS_ACT_*.  stats (optional, may be NULL): (n,2) zeroed doubles receiving
 * sum / sum of squares of y per sample (GroupNorm(1 group) statistics of the conv output).
 * The stride-1 input gradient is the same call on gy with mode-1 packed weights (cin/cout swapped). */
int dis_conv2d_fwd(const float* x, const float* w_packed, const float* bias, float* y, double* stats, int n,
                   int hin, int win, int cin, int cout, int k, int stride, int pad, int act, void* stream);
/* The same convolution for 3x3 stride-1 layers with 16 or 32 input and output channels (the FuseNet ResNet blocks; also
 * their input gradients with mode-1 weights) computed on the bf16 matrix cores at fp32 accuracy: every operand is split
 * into three bf16 terms (24 significant bits) and each product is accumulated as six bf16 x bf16 terms in the fp32 MFMA
 * accumulator; the dropped terms are <= 2^-24 relative, one fp32 rounding.
 * dis_conv2d_pack_bf16x3_size(cin, cout): 16-bit words of `packed` (negative: unsupported shape).
 * dis_conv2d_pack_weights_bf16x3: w_oihw is (cout, cin, 3, 3) for mode 0 and (cin, cout, 3, 3) for mode 1 (the weights
 * of the convolution whose input gradient is computed: channels swapped, taps flipped). */
long dis_conv2d_pack_bf16x3_size(int cin, int cout);
int dis_conv2d_pack_weights_bf16x3(const float* w_oihw, void* packed, int cout, int cin, int k, int mode, void* stream);
int dis_conv2d_fwd_bf16x3(const float* x, const void* w_packed, const float* bias, float* y, double* stats, int n, int hin,
                          int win, int cin, int cout, int k, int stride, int pad, int act, void* stream);
/* The same with the module's OIHW fp32 weights (w_o, w_i, 3, 3) handed over as they are: the kernel splits them into its
 * LDS-resident bf16 planes itself, which saves the packing launch per convolution call.  mode 0: forward (cout == w_o,
 * cin >= w_i: x may carry zero-padded extra channels); mode 1: input gradient of that convolution (cin == w_o,
 * cout >= w_i).  w_row_stride: floats between consecutive w_o rows (0 = dense = w_i*9; larger when w_oihw points at
 * w[:, a:b] inside a wider weight, as for the parts of a convolution over concatenated inputs). */
int dis_conv2d_fwd_bf16x3_oihw(const float* x, const float* w_oihw, int mode, int w_o, int w_i, int w_row_stride,
                               const float* bias, float* y, double* stats, int n, int hin, int win, int cin, int cout,
                               int k, int stride, int pad, int act, void* stream);
/* Input gradient of such a convolution when it was followed by an activation, with the activation's gradient fused in:
 * gx (+)= conv_T(gy * act'(y), w), y (same shape as gy) = the activation's output, w_oihw (w_o, w_i, 3, 3) the forward
 * weight (gy has cin == w_o channels, gx cout >= w_i).  Replaces dis_act_bwd + the mode-1 call above. */
int dis_conv2d_dgrad_bf16x3_act(const float* gy, const float* y, int act, const float* w_oihw, int w_o, int w_i,
                                int w_row_stride, float* gx, int n, int hin, int win, int cin, int cout, int pad,
                                int accumulate, void* stream);

/* dis_conv2d_fwd with per-pixel multipliers fused into the kernel (both optional, may be NULL):
 *   xscale (n,hin,win,NCHUNK): x[pixel][chunk c] is multiplied by xscale[pixel][c] while it is staged (NCHUNK = cin/32
 *          for cin % 32 == 0): conv(x * s) without materialising x * s;
 *   yscale (n,hout,wout,cout/32): the result (before bias / accumulation) of 32-channel group g is multiplied by
 *          yscale[pixel][g]: the input gradient of such a conv.
 * Used for the multi-frame 1x1 conv over the mask-weighted slots (reference multi_frame_networks.py:410-413) with
 * xscale = yscale = dis_slot_weights(geom). */
int dis_conv2d_fwd_scaled(const float* x, const float* xscale, const float* w_packed, const float* bias, float* y,
                          const float* yscale, double* stats, int n, int hin, int win, int cin, int cout, int k,
                          int stride, int pad, int act, void* stream);
/* wgt (pixels,tl) = mask / mean(mask) from geom (pixels,tl,4) */
int dis_slot_weights(const float* geom, float* wgt, long pixels, int tl, void* stream);

/* Weight/bias gradient.  gy: (n,hout,wout,cout) gradient wrt the PRE-activation output; x has cin_pad channels.
 * workspace: dis_conv2d_wgrad_workspace(cin_pad,cout,k,stride) floats (-1 if the shape is unsupported).
 * grad_w: (cout,cin_real,k,k) OIHW, grad_b: (cout) or NULL, both OVERWRITTEN.  Deterministic (partial slabs
 * per workgroup summed in a fixed order, no float atomics). */
long dis_conv2d_wgrad_workspace(int cin_pad, int cout, int k, int stride);
/* Round 6 - dis_conv2d_wgrad with gy * act'(y) formed while gy is staged (y = the conv's activated output): the layers whose input
 * gradient is never needed (FuseNet's stems conv1 4 -> 16 k4 s2 and amb_conv 4 -> 16 k3 s1, reference
 * model/multi_frame_networks.py:216-233) no longer need the dis_act_bwd pass.  workspace: dis_conv2d_wgrad_workspace(cin_pad, cout, k,
 * stride) floats.  DIS_ERR_UNSUPPORTED for any other shape. */
int dis_conv2d_wgrad_act(const float* x, const float* gy, const float* y, int act, float* grad_w, float* grad_b, float* workspace,
                         int n, int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad, void* stream);
/* Backward of the 1 x 1 multi-frame conv y = conv(x * xscale) (cin = 128 -> cout = 32) behind a GroupNorm in ONE launch:
 * dis_conv2d_dgrad1x1_scaled_gnb + dis_conv2d_wgrad_scaled without the stored operand gpre.  g, q (n, h, w, cout), coef from
 * dis_gn_bwd_coef, w_packed_dgrad the mode-1 packing of the weight; gx (n, h, w, cin) (+)= (gpre W^T) * yscale, bit-identical to
 * dis_conv2d_dgrad1x1_scaled_gnb's; grad_w (cout, cin, 1, 1), grad_b (cout) or NULL: per-workgroup slabs summed in fp64 in a fixed
 * order (no float atomics).  yscale / xscale (n, h, w, cin / 32) may be NULL.  workspace: dis_conv2d_bwd1x1_scaled_gnb_workspace(cin,
 * cout) floats (-1: no kernel for the shape).  DIS_ERR_UNSUPPORTED for any other shape and under DIS_MF_BWD_FUSED=0. */
long dis_conv2d_bwd1x1_scaled_gnb_workspace(int cin, int cout);
int dis_conv2d_bwd1x1_scaled_gnb(const float* g, const float* q, const float* coef, int in_act, const float* w_packed_dgrad,
                                 float* gx, const float* yscale, const float* x, const float* xscale, float* grad_w, float* grad_b,
                                 float* workspace, int n, int h, int w, int cout, int cin, int accumulate, void* stream);
/* dis_conv2d_wgrad of conv(x * xscale) (see dis_conv2d_fwd_scaled); xscale may be NULL */
int dis_conv2d_wgrad_scaled(const float* x, const float* xscale, const float* gy, float* grad_w, float* grad_b,
                            float* workspace, int n, int hin, int win, int cin_pad, int cin_real, int cout, int k,
                            int stride, int pad, void* stream);
/* bf16x3 form (fp32 accuracy on the bf16 matrix cores, transposing LDS reads) for k = 3, stride 1 and 16 / 32 channels on
 * either side; same arguments, workspace and determinism as dis_conv2d_wgrad. */
int dis_conv2d_wgrad_bf16x3(const float* x, const float* gy, float* grad_w, float* grad_b, float* workspace, int n,
                            int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad,
                            void* stream);
/* The same for a convolution that was followed by an activation (act = DIS_ACT_SELU / RELU): gy is the gradient wrt the
 * activation's OUTPUT y and the kernel stages gy * act'(y).  Replaces dis_act_bwd + dis_conv2d_wgrad_bf16x3. */
int dis_conv2d_wgrad_bf16x3_act(const float* x, const float* gy, const float* y, int act, float* grad_w, float* grad_b,
                                float* workspace, int n, int hin, int win, int cin_pad, int cin_real, int cout, int k,
                                int stride, int pad, void* stream);
int dis_conv2d_wgrad(const float* x, const float* gy, float* grad_w, float* grad_b, float* workspace, int n,
                     int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad,
                     void* stream);
/* Operand split of the dis_conv2d_*_bf16x3* entry points that take fp32 weights (round 3): 1 = two fp16 terms, 3 products per
 * MAC (22-bit operands, power-of-two block scaling; default), 0 = three bf16 terms, 6 products (>= 24 bits).  Process-wide;
 * DIS_CONV_SPLIT=bf16x3 | f16x2 sets the initial value.  Same arguments, layouts and workspaces either way. */
int dis_set_conv_split(int mode);
int dis_get_conv_split(void);
/* Diagnostics: writes the name of the kernel template family the most recent convolution entry point of this process launched
 * ("conv_f16x2_kernel<32,32>", "conv_bf16x3_kernel<32,32>", "conv_fwd_kernel (fp32 MFMA)", ...; "" if none since the last call
 * with clear != 0) into the HOST buffer `name` of `cap` bytes, NUL-terminated.  bench.py labels its per-call HIP-event times
 * with it, so that a `*_bf16x3*` call served by the two-term fp16 kernel is reported as such.  Not thread-safe, never read by a
 * compute path. */
int dis_last_kernel(char* name, int cap, int clear);
/* GroupNorm applied ON LOAD by the consuming convolution (round 3).  The reference chains Conv2d -> SELU -> GroupNorm(1, C) ->
 * Conv2d (ResNetBlock model/multi_frame_networks.py:514-542; Block2D3D conv1_1 -> conv1_2, conv2_1 -> conv2_2 :338-345) and
 * writes the normalised tensor between them; here x is the PRE-normalisation tensor and the consumer stages
 * x * (rstd * gamma_c) + (beta_c - rstd * gamma_c * mean) per sample (gn_stats (n, 2): fp64 sum / sum of squares as
 * dis_conv2d_fwd leaves them; gn_gamma / gn_beta (cin)), padding stays zero: bit for bit dis_gn_apply followed by
 * dis_conv2d_fwd_bf16x3_oihw / dis_conv2d_wgrad_bf16x3, without the read + write of the normalised tensor.
 * 3x3, stride 1, cin == cout in {16, 32}, w_oihw (w_o, w_i, 3, 3) dense or a row-strided slice; act NONE / SELU. */
int dis_conv2d_fwd_bf16x3_gn(const float* x, const double* gn_stats, const float* gn_gamma, const float* gn_beta,
                             float gn_eps, const float* w_oihw, int w_o, int w_i, int w_row_stride, const float* bias,
                             float* y, double* stats, int n, int hin, int win, int cin, int cout, int k, int stride,
                             int pad, int act, void* stream);
/* ... and its backward without the GroupNorm reduce pass: the input gradient g = conv_T(gy, w) of that conv also leaves, per
 * (sample, channel), the sums of g and of g * x over the pixels (x = gn_x: the GroupNorm's input, shaped like g) - one fp64 slot per
 * workgroup, ab_out (n, dis_conv2d_gnsums_slots(), 2, cin), ZEROED by the caller - and dis_gn_bwd_from_sums turns g, x and the sums
 * into the gradient wrt x (times act'(x) for in_act != 0), grad_gamma and grad_beta in ONE elementwise pass (reference backward of
 * torch.nn.GroupNorm(1, C), model/multi_frame_networks.py:338-345).  coef: n * (c + 2) + 4 n c + 2 floats of workspace.  Two-term fp16
 * kernels only: DIS_ERR_UNSUPPORTED under dis_set_conv_split(0) (dis_gn_apply_bwd remains the general form). */
long dis_conv2d_gnsums_slots(void);
int dis_conv2d_dgrad_bf16x3_gnsums(const float* gy, const float* w_oihw, int w_o, int w_i, int w_row_stride, float* g,
                                   const float* gn_x, double* ab_out, int n, int hin, int win, int cin, int cout, int pad,
                                   void* stream);
/* The same for the residual pattern out = SELU(GroupNorm(x2) + res) whose gradient arrives through the NEXT ResNetBlock's first conv
 * (reference model/multi_frame_networks.py:514-542): that conv's accumulating input-gradient launch computes, in place,
 * g = (g + conv_T(gy, w)) * selu'(act_y) (g arrives holding the next block's residual-branch gradient, act_y = out) and the sums of
 * g and g * gn_x (gn_x = x2); g then is the residual gradient of THIS block and, with dis_gn_bwd_from_sums(in_act = 0), gives the
 * gradient wrt x2 - no reduce pass, no separate residual-gradient write.  act_y == NULL: a plain GroupNorm output with TWO consumers
 * (Block2D3D's conv_mf GroupNorm, :338-345): g = g + conv_T(gy, w) in place, the sums of g and g * gn_x as above. */
int dis_conv2d_dgrad_bf16x3_gnsums_res(const float* gy, const float* w_oihw, int w_o, int w_i, int w_row_stride, float* g,
                                       const float* act_y, const float* gn_x, double* ab_out, int n, int hin, int win, int cin,
                                       int cout, int pad, void* stream);
/* ... and when the consumer of `out` is a conv with an activation of its own (final_conv, 32 -> 16 + SELU, :262-266):
 * g = conv_T(gy * selu'(y), w) * selu'(act_y), written; cin = 16 (gy / y channels), cout = 32 - or (round 5) cin = 32, cout = 16: the
 * 16-channel slice w[:, 32:48] of ref_conv (48 -> 32 + SELU, :248-256) behind amb_res2, w_row_stride = 48 * 9. */
int dis_conv2d_dgrad_bf16x3_act_gnsums_res(const float* gy, const float* y, const float* w_oihw, int w_o, int w_i,
                                           int w_row_stride, float* g, const float* act_y, const float* gn_x, double* ab_out,
                                           int n, int hin, int win, int cin, int cout, int pad, void* stream);
int dis_gn_bwd_from_sums(const float* g, const float* x, const double* stats, const float* gamma, const double* ab, int slots,
                         float* gx, float* grad_gamma, float* grad_beta, float* coef, int n, long hw, int c, float eps,
                         int in_act, void* stream);
/* Round 5: the two halves of dis_gn_bwd_from_sums as entry points of their own, and the input-gradient launch that applies the second
 * half on load (csrc/norm_act.hip, csrc/conv2d.hip; reference backward of GroupNorm(1, C) in front of a 3x3 conv,
 * model/multi_frame_networks.py:338-345, :514-542).
 *   dis_gn_bwd_coef: ab (n, slots, 2, c) -> coef: (n, c + 2) floats [k1_c..., kx, k0] followed (8-byte aligned) by n * 2c doubles
 *     (n * (c + 2) + 4 n c + 2 floats in all), grad_gamma / grad_beta (c); counter: one unsigned, ZERO on entry (zero again on exit).
 *   dis_gn_bwd_apply_coef: gx = act'(x) (g k1_c + x kx + k0) - the elementwise pass alone.
 *   dis_conv2d_dgrad_f16x2_gnb: gx (+)= conv_T(gpre, w) with gpre = act'(q) (g k1_c + q kx + k0) formed while g and q are staged,
 *     gpre also stored to gpre_out for the weight-gradient launch; optional channel-sum epilogue as dis_conv2d_dgrad_bf16x3_gnsums /
 *     _gnsums_res (ab_gn_x, ab_act_y, ab_out; all NULL: none).  3x3, stride 1, pad 1, c -> c, c in {16, 32}; two-term fp16 kernels only. */
/* Round 5: y = act(conv3x3(out) + bias), out = SELU(GroupNorm(x2) + res) formed while x2 and res are staged (dis_gn_apply's arithmetic,
 * bit for bit) and stored to `out` by the tiles that own each pixel: a ResNetBlock's output is written by the conv that consumes it
 * first (reference model/multi_frame_networks.py:514-542).  3x3 stride 1 pad 1; c -> c (c in {16, 32}; stats optional) or 32 -> 16 (no
 * stats); act SELU; two-term fp16 kernels only. */
int dis_conv2d_fwd_f16x2_gnres(const float* x2, const double* gn_stats, const float* gn_gamma, const float* gn_beta, float gn_eps,
                               const float* res, float* out, const float* w_oihw, int w_o, int w_i, int w_row_stride,
                               const float* bias, float* y, double* stats, int n, int hin, int win, int cin, int cout, int act,
                               void* stream);
/* ... and the same for the 1 x 1 multi-frame conv (128 -> 32 with slot weights, model/multi_frame_networks.py:406-413), whose input
 * gradient runs on the fp32 MFMA kernel: g (n, h, w, 32) the gradient wrt the GroupNorm's output, q the GroupNorm's input, coef
 * (n, 34); gx (n, h, w, 128) (+)= (gpre W^T) * yscale[pixel][32-channel group] (yscale may be NULL); gpre stored to gpre_out for
 * dis_conv2d_wgrad_scaled.  w_packed = dis_conv2d_pack_weights(mode 1). */
int dis_conv2d_dgrad1x1_scaled_gnb(const float* g, const float* q, const float* coef, int in_act, float* gpre_out,
                                   const float* w_packed, float* gx, const float* yscale, int n, int hin, int win, int cin,
                                   int cout, int accumulate, void* stream);
/* ... and for the 4 x 4 stride-2 pad-1 conv (32 -> 32, Block2D3D.conv2_1, :338-345): here the WEIGHT-gradient launch applies the pass
 * while it stages gy (every gy pixel belongs to one tile) and stores gpre for dis_conv2d_dgrad_strided.  g / q (n, hout, wout, 32),
 * coef (n, 34), x (n, hin, win, 32); workspace: dis_conv2d_wgrad_workspace(32, 32, 4, 2) floats.  Two-term fp16 kernel only. */
int dis_conv2d_wgrad_k4s2_f16x2_gnb(const float* x, const float* g, const float* q, const float* coef, int in_act, float* gpre_out,
                                    float* grad_w, float* grad_b, float* workspace, int n, int hin, int win, void* stream);
/* Round 5: FuseNet's 4 x 4 stride-2 pad-1 down convolution (32 -> 32, Block2D3D.conv2_1, model/multi_frame_networks.py:338-345)
 * forward on the two-term fp16 kernels (csrc/conv_k4s2.hip: wave-resident weights, de-interleaved halo columns): y = act(conv(x, w) +
 * bias), w OIHW (32, 32, 4, 4) unpacked, stats (n, 2) accumulated or NULL.  DIS_ERR_UNSUPPORTED under dis_set_conv_split(0). */
int dis_conv2d_fwd_k4s2_f16x2(const float* x, const float* w_oihw, const float* bias, float* y, double* stats, int n, int hin, int win,
                              int act, void* stream);
/* ... and its input gradient: gx (n, hin, win, 32) (+)= conv_transpose(gy (n, hin / 2, win / 2, 32), w), the four parity classes from
 * one gy halo tile in one launch (replaces dis_conv2d_dgrad_strided's four launches + four packing launches); hin, win even. */
int dis_conv2d_dgrad_k4s2_f16x2(const float* gy, const float* w_oihw, float* gx, int n, int hin, int win, int accumulate, void* stream);
/* Round 5: the channel sums dis_gn_bwd_coef starts from when NO convolution epilogue left them (the gradient wrt the GroupNorm's output
 * arrives from a join, a resize or a feature warp: Block2D3D's conv_fuse GroupNorm with its residual, model/multi_frame_networks.py
 * :338-345, FuseNet.res3's last GroupNorm, :514-542): g = gy * act'(y) (y / act: the GroupNorm output's activation; NULL / 0: g = gy),
 * g stored to gres when given (the residual gradient), ab_out (n, slots, 2, c) doubles = per-block sums of g and g * x, every slot
 * written.  With dis_gn_bwd_coef and an on-load elementwise pass this replaces dis_gn_apply_bwd's reduce + apply launches. */
int dis_gn_bwd_res_sums(const float* gy, const float* y, const float* x, float* gres, double* ab_out, int slots, int n, long hw, int c,
                        int act, void* stream);
int dis_gn_bwd_coef(const double* stats, const float* gamma, const double* ab, int slots, float* coef, float* grad_gamma,
                    float* grad_beta, unsigned* counter, int n, long hw, int c, float eps, void* stream);
int dis_gn_bwd_apply_coef(const float* g, const float* x, const float* coef, float* gx, int n, long hw, int c, int in_act,
                          void* stream);
int dis_conv2d_dgrad_f16x2_gnb(const float* g, const float* q, const float* coef, int in_act, float* gpre_out, const float* w_oihw,
                               int w_o, int w_i, int w_row_stride, float* gx, int accumulate, const float* ab_gn_x,
                               const float* ab_act_y, double* ab_out, int n, int hin, int win, int c, void* stream);
/* Round 6 - input gradient AND weight gradient of a 3x3 stride-1 pad-1 conv c -> c (c = 32) in ONE launch (csrc/conv_bwd_fused.hip):
 * replaces the pair dis_conv2d_dgrad_f16x2_gnb / dis_conv2d_fwd_bf16x3_oihw(mode 1) + dis_conv2d_wgrad_bf16x3[_gn | _act] of one Conv2d
 * node (reference: torch.nn.Conv2d's backward inside ResNetBlock / Block2D3D, model/multi_frame_networks.py:338-345,514-542).
 *   operand of both products: coef != NULL: gpre = act'(q) (g k1_c + q kx + k0), as dis_conv2d_dgrad_f16x2_gnb forms it (also stored to
 *     gpre_out when that is non-NULL); coef == NULL: g (in_act == 0) or g act'(q) (q = the conv's activated output).
 *   input gradient gx: dis_conv2d_dgrad_f16x2_gnb's forms (accumulate, ab_gn_x / ab_act_y / ab_out) - bit-identical results.
 *   weight gradient: x (n, hin, win, c) = the conv's input; x_gn_stats != NULL: staged as GroupNorm(x) (dis_conv2d_wgrad_bf16x3_gn);
 *     x may be the tensor ab_gn_x or ab_act_y (fetched once).  grad_w (c, c, 3, 3), rows grad_w_row_stride floats apart (0 = contiguous;
 *     a multiple of 9 >= 9 c: the slice of a wider OIHW gradient, e.g. of a conv over a channel concatenation), grad_b (c) or NULL;
 *     workspace: dis_conv2d_bwd_fused_workspace(c) floats (-1: no kernel for this channel count).
 * DIS_ERR_UNSUPPORTED: no instance for the combination / the three-term mode / DIS_BWD_FUSED=0 (the caller keeps the two launches). */
long dis_conv2d_bwd_fused_workspace(int c);
int dis_conv2d_bwd_fused_f16x2(const float* g, const float* q, const float* coef, int in_act, float* gpre_out, const float* w_oihw,
                               int w_o, int w_i, int w_row_stride, float* gx, int accumulate, const float* ab_gn_x,
                               const float* ab_act_y, double* ab_out, const float* x, const double* x_gn_stats,
                               const float* x_gn_gamma, const float* x_gn_beta, float x_gn_eps, float* grad_w, float* grad_b,
                               float* workspace, int n, int hin, int win, int c, int grad_w_row_stride, void* stream);
/* The same ONE launch for the 3x3 stride-1 pad-1 layers with 16 channels on a side (csrc/conv_bwd_fused_c16.hip for 16 -> 16,
 * csrc/conv_bwd_fused_mixed.hip for 16 -> 32 and 32 -> 16): w_oihw is
 * (w_o, w_i, 3, 3), g / q / gpre_out have w_o channels, x / gx / ab_gn_x / ab_act_y w_i.  Operand, input-gradient forms (gx BIT-identical
 * to the two launches'), x / x_gn_*, grad_w (rows grad_w_row_stride floats apart, 0 = contiguous) and grad_b (w_o) as
 * dis_conv2d_bwd_fused_f16x2.  A mixed pair has two forms, both with the operand g selu'(q) (coef NULL, in_act SELU) and
 * accumulate == 0: all of ab_* NULL (gx = conv_T(.)), or ab_act_y == x with ab_gn_x and ab_out (gx = conv_T(.) selu'(x), WRITTEN, and
 * the channel sums of gx and gx ab_gn_x: dis_conv2d_dgrad_bf16x3_act_gnsums_res's arithmetic).
 * The kernel runs dis_conv2d_bwd_fused_c16_slots(w_i, w_o) workgroups at most (two per CU for 16 -> 16, one for a mixed pair):
 *   workspace: dis_conv2d_bwd_fused_c16_workspace(w_i, w_o) floats (-1: no kernel for this pair of channel counts);
 *   ab_out: (n, ab_slots, 2, w_i) doubles, ZEROED by the caller, one slot per workgroup - ab_slots is the caller's slot count (what it
 *     hands to dis_gn_bwd_coef); a launch with channel sums runs min(ab_slots, dis_conv2d_bwd_fused_c16_slots()) workgroups.
 * DIS_ERR_UNSUPPORTED: no instance for the combination / the three-term mode / DIS_BWD_FUSED=0 (the caller keeps the two launches). */
long dis_conv2d_bwd_fused_c16_workspace(int cin, int cout);
long dis_conv2d_bwd_fused_c16_slots(int cin, int cout);
int dis_conv2d_bwd_fused_f16x2_c16(const float* g, const float* q, const float* coef, int in_act, float* gpre_out, const float* w_oihw,
                                   int w_o, int w_i, int w_row_stride, float* gx, int accumulate, const float* ab_gn_x,
                                   const float* ab_act_y, double* ab_out, int ab_slots, const float* x, const double* x_gn_stats,
                                   const float* x_gn_gamma, const float* x_gn_beta, float x_gn_eps, float* grad_w, float* grad_b,
                                   float* workspace, int n, int hin, int win, int grad_w_row_stride, void* stream);
/* Input gradient AND weight gradient of a 3x3 stride-1 pad-1 conv c -> c (c = 32) in ONE launch under the three-term bf16 split
 * (csrc/conv_bwd_fused_bf16x3.hip): six bf16 products per MAC, fp32 accumulation.  Replaces the strict mode's pair
 * dis_conv2d_fwd_bf16x3_oihw(mode 1) | dis_conv2d_dgrad_bf16x3_act + dis_conv2d_wgrad_bf16x3 | _act | _gn of one Conv2d node.
 * Forms (the signature is dis_conv2d_bwd_fused_f16x2's without coef / gpre_out / ab_*):
 *   plain: operand g (in_act == 0); gx = conv_T(g, w), or gx += it (accumulate != 0).
 *   act:   operand g * SELU'(q) (in_act == DIS_ACT_SELU, q = the conv's activated output), formed on load; gx written or accumulated.
 *   xgn:   x_gn_stats != NULL (with gamma, beta, eps): the weight gradient stages GroupNorm(x) as dis_conv2d_wgrad_bf16x3_gn does;
 *          the gx side is plain, not accumulating.
 *   gx is BIT-identical to dis_conv2d_fwd_bf16x3_oihw(mode 1) (plain) and dis_conv2d_dgrad_bf16x3_act (act) on the same operands.
 *   weight gradient: x (n, hin, win, c) = the conv's input; grad_w (c, c, 3, 3), rows grad_w_row_stride floats apart (0 = contiguous;
 *     a multiple of 9 >= 9 c: the slice of a wider OIHW gradient), grad_b (c) or NULL.  Per-workgroup slabs in the caller-owned
 *     workspace of dis_conv2d_bwd_fused_bf16x3_workspace(c) floats (-1: no kernel for this channel count), reduced in a fixed order:
 *     no float atomics, bit-reproducible.
 * DIS_ERR_UNSUPPORTED: under the two-term split (dis_get_conv_split() == 1), with DIS_BWD_FUSED=0, and for any combination without an
 * instance (another channel count, another activation, xgn with in_act or accumulate): the caller keeps the two launches. */
long dis_conv2d_bwd_fused_bf16x3_workspace(int c);
int dis_conv2d_bwd_fused_bf16x3(const float* g, const float* q, int in_act, const float* w_oihw, int w_o, int w_i, int w_row_stride,
                                float* gx, int accumulate, const float* x, const double* x_gn_stats, const float* x_gn_gamma,
                                const float* x_gn_beta, float x_gn_eps, float* grad_w, float* grad_b, float* workspace, int n,
                                int hin, int win, int c, int grad_w_row_stride, void* stream);
int dis_conv2d_wgrad_bf16x3_gn(const float* x, const double* gn_stats, const float* gn_gamma, const float* gn_beta,
                               float gn_eps, const float* gy, float* grad_w, float* grad_b, float* workspace, int n,
                               int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad,
                               void* stream);
/* Split-neutral names (round 5) of the 3x3 entry points above whose `_bf16x3` suffix is history: which operand split multiplies is a
 * process-wide mode (dis_set_conv_split: 1 = two-term fp16, 3 products per MAC, the default; 0 = three-term bf16, 6 products, >= 24-bit
 * operands), not a property of the entry point.  Same symbols' code (ELF aliases), same arguments. */
int dis_conv2d_fwd_split_oihw(const float* x, const float* w_oihw, int mode, int w_o, int w_i, int w_row_stride, const float* bias, float* y, double* stats, int n, int hin, int win, int cin, int cout, int k, int stride, int pad, int act, void* stream);
int dis_conv2d_fwd_split_gn(const float* x, const double* gn_stats, const float* gn_gamma, const float* gn_beta, float gn_eps, const float* w_oihw, int w_o, int w_i, int w_row_stride, const float* bias, float* y, double* stats, int n, int hin, int win, int cin, int cout, int k, int stride, int pad, int act, void* stream);
int dis_conv2d_dgrad_split_gnsums(const float* gy, const float* w_oihw, int w_o, int w_i, int w_row_stride, float* g, const float* gn_x, double* ab_out, int n, int hin, int win, int cin, int cout, int pad, void* stream);
int dis_conv2d_dgrad_split_gnsums_res(const float* gy, const float* w_oihw, int w_o, int w_i, int w_row_stride, float* g, const float* act_y, const float* gn_x, double* ab_out, int n, int hin, int win, int cin, int cout, int pad, void* stream);
int dis_conv2d_dgrad_split_act_gnsums_res(const float* gy, const float* y, const float* w_oihw, int w_o, int w_i, int w_row_stride, float* g, const float* act_y, const float* gn_x, double* ab_out, int n, int hin, int win, int cin, int cout, int pad, void* stream);
int dis_conv2d_dgrad_split_act(const float* gy, const float* y, int act, const float* w_oihw, int w_o, int w_i, int w_row_stride, float* gx, int n, int hin, int win, int cin, int cout, int pad, int accumulate, void* stream);
int dis_conv2d_wgrad_split(const float* x, const float* gy, float* grad_w, float* grad_b, float* workspace, int n, int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad, void* stream);
int dis_conv2d_wgrad_split_act(const float* x, const float* gy, const float* y, int act, float* grad_w, float* grad_b, float* workspace, int n, int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad, void* stream);
int dis_conv2d_wgrad_split_gn(const float* x, const double* gn_stats, const float* gn_gamma, const float* gn_beta, float gn_eps, const float* gy, float* grad_w, float* grad_b, float* workspace, int n, int hin, int win, int cin_pad, int cin_real, int cout, int k, int stride, int pad, void* stream);

/* Input gradient of a k=4, stride=2, pad=1 convolution (transposed convolution) as four 2x2 phase convolutions on
 * the matrix cores.  w_oihw is the unpacked weight (cout,cin,4,4).  workspace: 16*cin*cout floats.
 * gx: (n,hin,win,cin) overwritten, or added to when `accumulate` != 0. */
int dis_conv2d_dgrad_strided(const float* gy, const float* w_oihw, float* gx, float* workspace, int n, int hin,
                             int win, int cin, int cout, int k, int stride, int pad, int accumulate, void* stream);

/* Head: Conv2d(cin,1,3,pad 1) + alpha*sigmoid(x - offset) (reference networks.py:121-125,140-149;
 * multi_frame_networks.py:157,265), cin = 16 or 32.  x nhwc (n,h,w,cin); w (1,cin,3,3); y planar (n,1,h,w). */
int dis_disp_head_fwd(const float* x, const float* w, const float* b, float* y, int n, int h, int wd, int cin,
                      float alpha, float offset, void* stream);
/* gy (n,1,h,w) gradient wrt y; y is the forward output.  gx (n,h,w,cin) overwritten; grad_w/grad_b overwritten.
 * workspace: dis_disp_head_bwd_workspace(n,h,wd,cin) floats (8-byte aligned: pre-sigmoid gradient + fp64 block slabs). */
long dis_disp_head_bwd_workspace(int n, int h, int wd, int cin);
int dis_disp_head_bwd(const float* x, const float* w, const float* y, const float* gy, float* gx, float* grad_w,
                      float* grad_b, float* workspace, int n, int h, int wd, int cin, float alpha, void* stream);

/* dy *= act'(y) given the activation OUTPUT y (SELU and ReLU are invertible enough for that). In place ok. */
int dis_act_bwd(const float* gy, const float* y, float* gpre, int act, long count, void* stream);
/* The same on channel ranges of wider nhwc buffers: gy / y pixels are ldg / ldy floats apart (c % 4 == 0, 16-byte
 * aligned), gpre is dense (npix, c); act == DIS_ACT_NONE gathers gy.  Host side: ops._ConvG.backward when a layer's
 * output lives inside a decoder concatenation buffer (the reference concatenates with torch.cat, networks.py:262-288). */
int dis_act_bwd_ld(const float* gy, int ldg, const float* y, int ldy, float* gpre, int act, long npix, int c,
                   void* stream);
/* dis_act_bwd_ld + the bias gradient bias_grad[ch] = sum_pixels gpre[pixel][ch] from the same pass (fp32 block partials, fp64
   totals, fixed order); workspace: dis_act_bwd_ld_bias_workspace(c) floats; c / 4 must divide 256, else DIS_ERR_UNSUPPORTED */
long dis_act_bwd_ld_bias_workspace(int c);
int dis_act_bwd_ld_bias(const float* gy, int ldg, const float* y, int ldy, float* gpre, int act, long npix, int c,
                        float* bias_grad, float* workspace, void* stream);
/* dst[pixel*ldd + j] = src[pixel*lds + j] for j < c and 0 for c <= j < c + czero: a tensor written into a channel range
 * of a wider nhwc buffer, followed by czero zero lanes (the padding of a concatenation to a multiple of 4 channels). */
int dis_copy_channels(const float* src, int lds, float* dst, int ldd, long npix, int c, int czero, void* stream);

/* GroupNorm(num_groups=1) statistics: stats (n,2) zeroed doubles <- sum, sumsq over (h,w,c) per sample. */
int dis_gn_stats(const float* x, double* stats, int n, long per_sample, void* stream);
/* y = act( gamma_c*(x-mean)*rstd + beta_c (+ residual) );  nhwc, eps 1e-5 (torch default).
 * Covers GroupNorm of reference multi_frame_networks.py:336,344,451,522,526 and the residual tail :539-540. */
int dis_gn_apply(const float* x, const double* stats, const float* gamma, const float* beta, const float* residual,
                 float* y, int n, long hw, int c, int act, float eps, void* stream);
/* Backward of dis_gn_apply.  gy: grad wrt y; y: forward output (needed when act != none); x: forward input.
 * red / gparam_acc: workspaces for per-block partial sums (no zeroing needed, no atomics; summed in a fixed order):
 * with W = dis_gn_bwd_workspace(n,c) doubles in total, red = W*2/(2+2c) doubles and gparam_acc = W*2c/(2+2c) doubles
 * (i.e. n*64*2 and n*64*2c).
 * gx overwritten; gres (optional) receives the residual-branch gradient (= gradient after act');
 * grad_gamma/grad_beta (c floats) overwritten.
 * in_act != DIS_ACT_NONE: x is the activation OUTPUT of the producing layer (conv -> SELU -> GroupNorm, reference
 * multi_frame_networks.py:338-345,533-535) and gx is additionally multiplied by act'(x), i.e. it is the gradient wrt
 * that layer's PRE-activation output (saves the separate dis_act_bwd pass). */
long dis_gn_bwd_workspace(int n, int c);
int dis_gn_apply_bwd(const float* gy, const float* y, const float* x, const double* stats, const float* gamma,
                     float* gx, float* gres, float* grad_gamma, float* grad_beta, double* red, double* gparam_acc,
                     int n, long hw, int c, int act, float eps, int in_act, void* stream);

/* y = act(a + b) elementwise and its backward (residual SELU of Block2D3D, reference :428). */
int dis_add_act_fwd(const float* a, const float* b, float* y, int act, long count, void* stream);

/* Scale the tl slots of a gathered feature tensor by mask/mean(mask) (reference multi_frame_networks.py:410):
 * wf (tl,bs,h,w,tl,c); geom (tl,bs,h,w,tl,4) (mask in .w); out same shape as wf.  Backward is the same call on
 * the gradient; accumulate != 0 adds the result to `out` instead of overwriting it. */
int dis_mask_weight_slots(const float* wf, const float* geom, float* out, long pixels, int tl, int c, int accumulate,
                          void* stream);

/* ---------------------------------------------------------------- Conv3D (k-NN continuous conv) */

/* reference multi_frame_networks.py:469-512 for ALL target frames at once, in two stages.
 * geom: (tl,bs,h,w,tl,4) xyz+mask per slot; wf: (tl,bs,h,w,tl,c) gathered features (c == 32).
 * tl: the track length, 2, 3 or 4 (the kernels are instanced per track length) in every dis_conv3d_* entry point; any other
 * value returns DIS_ERR_UNSUPPORTED (-1 from the size queries).
 *
 * stage 1, neighbour selection (reference :489-498): per output pixel the 9 candidates with the smallest masked
 * planar distance among the 3x3 x tl window (candidate id = (ky*3+kx)*tl+slot, zero-padded border).
 * idx_out: (tl,bs,ho,wo,9) uint8.  Ties / masked fills resolve to the lowest candidate id (the reference leaves
 * them to torch.topk(sorted=False), i.e. implementation-defined).  The selection depends on the geometry
 * only, so one call serves every Conv3D layer that shares `geom`. */
int dis_conv3d_knn_select(const float* geom, unsigned char* idx_out, int tl, int bs, int h, int wd, int stride,
                          void* stream);
/* stage 2 (reference :499-508): gather, MLP 3->16->32 on the local coordinates, weighted feature sum, 32x32 mix,
 * SELU.  dense1_w (16,3), dense1_b (16), dense2_w (32,16), dense2_b (32), w (32,32).
 * y: (tl,bs,ho,wo,32) = SELU(agg @ w)  (GroupNorm follows as dis_gn_*). */
int dis_conv3d_knn_fwd(const float* geom, const float* wf, const float* dense1_w, const float* dense1_b,
                       const float* dense2_w, const float* dense2_b, const float* w, const unsigned char* idx,
                       float* y, int tl, int bs, int h, int wd, int stride, void* stream);
/* The forward that also keeps agg (tl,bs,ho,wo,32), the weighted feature sums in front of the 32x32 mix, for
 * dis_conv3d_knn_bwd_det (agg may be NULL: dis_conv3d_knn_fwd). */
int dis_conv3d_knn_fwd_agg(const float* geom, const float* wf, const float* dense1_w, const float* dense1_b,
                           const float* dense2_w, const float* dense2_b, const float* w, const unsigned char* idx,
                           float* y, float* agg, int tl, int bs, int h, int wd, int stride, void* stream);
/* Round 2's backward (recomputes agg), kept as the reference the tests hold dis_conv3d_knn_bwd_det to: the package does not
 * call it.  gy: gradient wrt y (post-SELU).  grad_wf (zeroed) scatter-added (float atomics, 128-B rows).  gparams:
 * 32*32+16*3+16+32*16+32 floats overwritten in that order (w, dense1_w, dense1_b, dense2_w, dense2_b: the order of
 * the module's parameters()).
 * workspace: dis_conv3d_knn_bwd_workspace() floats (per-block partial slabs, summed in a fixed order). */
long dis_conv3d_knn_bwd_workspace(void);
int dis_conv3d_knn_bwd(const float* geom, const float* wf, const float* dense1_w, const float* dense1_b,
                       const float* dense2_w, const float* dense2_b, const float* w, const unsigned char* idx,
                       const float* y, const float* gy, float* grad_wf, float* gparams, float* workspace, int tl,
                       int bs, int h, int wd, int stride, void* stream);

/* The backward of Conv3D (reference :469-512 under autograd) with a DETERMINISTIC feature gradient and no index structure:
 * the output pixels are processed in 9 (stride 1) / 4 (stride 2) classes of pixels with pairwise disjoint 3x3 windows, one
 * launch per class, so the rows of grad_wf are updated with plain read-modify-writes in a fixed order.  grad_wf is ADDED to
 * (zero it, or hand in the gradient another consumer of wf has written).  agg: from dis_conv3d_knn_fwd_agg.  gparams as above.
 * workspace: dis_conv3d_knn_bwd_det_workspace(...) floats. */
long dis_conv3d_knn_bwd_det_workspace(int tl, int bs, int h, int wd, int stride);
int dis_conv3d_knn_bwd_det(const float* geom, const float* wf, const float* dense1_w, const float* dense1_b,
                           const float* dense2_w, const float* dense2_b, const float* w, const unsigned char* idx,
                           const float* y, const float* agg, const float* gy, float* grad_wf, float* gparams,
                           float* workspace, int tl, int bs, int h, int wd, int stride, void* stream);

/* ---------------------------------------------------------------- general convolution family (DIS-SF) */

/* Streaming implicit-GEMM convolution on the matrix cores for the DispNetS encoder-decoder (reference
 * model/networks.py:170-295: Conv2d k7/k5/k3 stride 1/2 with ReLU :222-234, ConvTranspose2d(k3,s2,p1,op1) :236-240
 * with crop_like :242-244), channel counts 2..1024.  All tensors nhwc; a tensor argument is (pointer, ld, off):
 * a pixel occupies `ld` floats and the channels [off, off+c) are used, so channel slices of a concatenated buffer
 * can be read / written in place.  `cin`/`cout` are the channel counts processed (cin % 4 == 0); `cin_w`/`cout_w`
 * (<= cin/cout) are the channels the weight tensor really has: the rest are zero-padded lanes (read as zero weights,
 * written as zeros).
 *   DIS_CONVG_CONV        y = act(conv(x, w[cout_w][cin_w][k][k]) + bias), hout = (hin+2*pad-k)/stride+1
 *   DIS_CONVG_CONV_DGRAD  x := gradient wrt the conv's pre-activation output (n,hin,win,cin = conv cout);
 *                         y := gradient wrt the conv's input (n,hout,wout,cout = conv cin); w is the conv's weight
 *                         [cin_w][cout_w][k][k]; stride 2 runs as 4 output-parity phases
 *   DIS_CONVG_TCONV       y = act(conv_transpose(x, w[cin_w][cout_w][k][k], stride 2) + bias) cropped to (hout,wout)
 *   DIS_CONVG_TCONV_DGRAD x := gradient wrt the (cropped) transposed-conv output; y := gradient wrt its input;
 *                         w is the transposed conv's weight [cout_w][cin_w][k][k]
 * wpack: workspace of dis_convg_pack_workspace(cin,cout,k) floats (x4 for the two phase-decomposed cases:
 * CONV_DGRAD and TCONV with stride 2) PLUS dis_convg_splitk_workspace(...) floats (round 4; 0 for most calls: partial sums of
 * the split-K form small maps take under the two-term fp16 split).
 * Routing (same results, same contract): 3x3 stride-1 CONV / CONV_DGRAD calls with <= 10 32x32 channel-slice launches and
 * >= 400k pixels run on the halo-resident kernels (7x7 too, one launch per tap row, under the three-term split); with >= 32 input
 * channels and a virtual output grid of >= 1024 positions (DIS_CONVG_HALO_MIN) the call takes the LDS-halo form convh2_kernel
 * (round 4: the input halo of a tile staged once per 32-channel chunk, all taps from LDS; the four parity phases of the stride-2
 * transposed forms in one launch when their weights stay resident); everything else streams (256 x 128 tiles for >= 128 channels
 * on both sides).
 * Arithmetic (dis_set_conv_split, default 1): layers with >= 32 input channels multiply two-term fp16 operands (3 products per
 * MAC, fp32 accumulate; one power-of-two scale per image of x in the streaming kernel, per halo tile in the slice launches and in
 * the halo form, and one per weight tensor); dis_set_conv_split(0) selects the three-term bf16 split (6 products, >= 24-bit operands) everywhere. */
#define DIS_CONVG_CONV 0
#define DIS_CONVG_CONV_DGRAD 1
#define DIS_CONVG_TCONV 2
#define DIS_CONVG_TCONV_DGRAD 3
long dis_convg_pack_workspace(int cin, int cout, int k);
long dis_convg_splitk_workspace(int mode, int n, int hin, int win, int hout, int wout, int cin, int cout, int k, int stride,
                                int pad);
int dis_convg_run(int mode, const float* x, int ldx, int xoff, const float* w, const float* bias, float* y, int ldy,
                  int yoff, float* wpack, int n, int hin, int win, int cin, int cin_w, int hout, int wout, int cout,
                  int cout_w, int k, int stride, int pad, int act, void* stream);

/* Weight gradient of the family: grad_w[g][x][ky][kx] = sum_{n,gy,gx} X[n][gy*stride-pad+ky][gx*stride-pad+kx][x] *
 * G[n][gy][gx][g]  (g < cG_w, x < cX_w; OVERWRITTEN; deterministic split-K slabs).
 *   conv:            X = layer input,              G = gradient wrt the pre-activation output  -> (cout,cin,k,k)
 *   transposed conv: X = gradient wrt its output,  G = layer input                             -> (cin,cout,k,k)
 * workspace: dis_convg_wgrad_workspace(n,hG,wG,cX,cG,k) floats.
 * Routing: k in {3,5} with stride in {1,2} and k = 7 with stride 1, cX >= 16, cG >= 32 run as 32x32 channel-slice pairs of the one-pass
 * halo kernels (x and G staged once for all taps; two-term fp16 operands by default, the three-term bf16 split under
 * dis_set_conv_split(0)); other shapes on the fp32 split-K kernel (one pass per tap). */
long dis_convg_wgrad_workspace(int n, int hG, int wG, int cX, int cG, int k);
int dis_convg_wgrad(const float* X, int ldX, int xoff, int hX, int wX, int cX, int cX_w, const float* G, int ldG,
                    int goff, int hG, int wG, int cG, int cG_w, float* grad_w, float* workspace, int n, int k,
                    int stride, int pad, void* stream);

/* out[c] = sum over npix pixels of G[pixel*ldG + goff + c]  (bias gradients).  workspace: dis_colsum_workspace(c). */
long dis_colsum_workspace(int c);
int dis_colsum(const float* G, int ldG, int goff, long npix, int c, float* out, float* workspace, void* stream);

/* SigmoidAffine of the DIS-SF disparity heads, reference model/networks.py:140-149: y = alpha*sigmoid(x - offset).
 * The backward writes the pre-sigmoid gradient as a zero-padded 4-channel nhwc tensor (count,4) for dis_convg_*. */
int dis_sigmoid_affine_fwd(const float* x, float* y, float alpha, float offset, long count, void* stream);
int dis_sigmoid_affine_bwd(const float* y, const float* gy, float* gpre4, float alpha, long count, void* stream);

/* ---------------------------------------------------------------- DispNetS, bf16 activation storage -------- */

/* BASELINE config 2 ("DIS-SF bs=8 ... bf16"): the encoder-decoder's nhwc feature maps are stored as bf16, convolutions
 * are ONE bf16 x bf16 product per MAC with fp32 accumulation; parameters, their gradients, disparities and losses stay
 * fp32.  Same modes / argument meaning as dis_convg_run and dis_convg_wgrad (reference model/networks.py:170-295:
 * Conv2d k7/k5/k3 s1/s2 + ReLU, ConvTranspose2d(k3,s2,p1,op1) + crop_like), with a storage flag per tensor
 * (x_bf16 / y_bf16 / g_bf16: 1 = bf16, 0 = fp32) and ld / channel offsets counted in ELEMENTS of the tensor's own
 * type (bf16: multiples of 8, fp32: multiples of 4).  dis_convb_pack_workspace counts 16-bit words per phase (x4);
 * wpack holds 4 x that many words PLUS dis_convb_splitk_workspace(...) floats (round 4; 0 for most calls: partial sums of the
 * split-K form the small maps of the deep layers take). */
long dis_convb_pack_workspace(int cin, int cout, int k);
long dis_convb_splitk_workspace(int mode, int x_bf16, int n, int hin, int win, int hout, int wout, int cin, int cout, int k,
                                int stride, int pad);
/* One packing launch per step (round 4).  A call's packed weights depend on its weights alone, which change once per step:
 *   dis_convb_pack_record(host_descs, capacity, NULL)  every packing launch of the dis_convb_run calls that follow also leaves a
 *                                                      descriptor (dis_convb_pack_desc_bytes() bytes) in the HOST array;
 *   dis_convb_pack_record(NULL, 0, out)                stops; out[0] = descriptors seen (> capacity: the record is incomplete,
 *                                                      do not use it), out[1] = workgroups of the batch launch (its plan is
 *                                                      written into the descriptors: upload them AFTER the stop);
 *   dis_convb_pack_batch(dev_descs, count, workgroups, stream)  packs all recorded calls' weights (into the wpack buffers they were
 *                                                      recorded with: the caller keeps those alive and unchanged) in ONE launch;
 *   dis_convb_run(mode | DIS_CONVB_PREPACKED, ...)     runs a recorded call on its packed weights (w may be NULL).
 * The record is process-global host state (like dis_last_kernel), not thread-safe. */
#define DIS_CONVB_PREPACKED 0x100
long dis_convb_pack_desc_bytes(void);
int dis_convb_pack_record(void* host_descs, int capacity, int* count_out);
int dis_convb_pack_batch(const void* dev_descs, int count, int workgroups, void* stream);
int dis_convb_run(int mode, const void* x, int x_bf16, int ldx, int xoff, const float* w, const float* bias, void* y,
                  int y_bf16, int ldy, int yoff, void* wpack, int n, int hin, int win, int cin, int cin_w, int hout,
                  int wout, int cout, int cout_w, int k, int stride, int pad, int act, void* stream);
long dis_convb_wgrad_workspace(int n, int hG, int wG, int cX, int cG, int k);
int dis_convb_wgrad(const void* X, int x_bf16, int ldX, int xoff, int hX, int wX, int cX, int cX_w, const void* G,
                    int g_bf16, int ldG, int goff, int hG, int wG, int cG, int cG_w, float* grad_w, float* workspace, int n,
                    int k, int stride, int pad, void* stream);
/* gpre = gy * act'(y) on channel ranges (ldg / ldy elements per pixel) of bf16 nhwc buffers; gpre dense (npix, c) bf16 */
int dis_act_bwd_bf16(const void* gy, int ldg, const void* y, int ldy, void* gpre, int act, long npix, int c,
                     void* stream);
/* dis_act_bwd_bf16 + the bias gradient bias_grad[ch] = sum_pixels gpre[pixel][ch] from the same pass (summed in fp32 before gpre's
   rounding); workspace: dis_colsum_bf16_workspace(c) floats; c / 4 must divide 256, else DIS_ERR_UNSUPPORTED */
int dis_act_bwd_bf16_bias(const void* gy, int ldg, const void* y, int ldy, void* gpre, int act, long npix, int c,
                          float* bias_grad, float* workspace, void* stream);
/* the same with a dense fp32 result (the network's first layer: x is fp32, its weight gradient runs through dis_conv2d_wgrad) */
int dis_act_bwd_bf16_f32(const void* gy, int ldg, const void* y, int ldy, float* gpre, int act, long npix, int c,
                         void* stream);
/* dis_copy_channels into a bf16 buffer from an fp32 (src_bf16 = 0) or bf16 source */
int dis_copy_channels_bf16(const void* src, int src_bf16, int lds, void* dst, int ldd, long npix, int c, int czero,
                           void* stream);
/* dis_colsum of a bf16 tensor (bias gradients), fp32 result */
long dis_colsum_bf16_workspace(int c);
int dis_colsum_bf16(const void* G, int ldG, int goff, long npix, int c, float* out, float* workspace, void* stream);

/* ---------------------------------------------------------------- augmentation -------------- */

/* Training-time augmentation of the IR and ambient images on the device (reference data/data_manipulation.py:114-195 with
 * data/dataset.py:67-70: no affine part, 5x5 Gaussian blur sigma in [0.2,0.5], Gaussian noise <= 3/255, salt-and-pepper
 * <= 5e-4, clip to [0,1]).  im / amb / outputs: (n, h, w) planes.  params: n x 6 floats on the DEVICE
 * {blur flag, sigma_im, sigma_amb, noise_im, noise_amb, sp_ratio or < 0}; seed: one int64 on the device (both may be
 * static buffers of a captured step); minmax_ws: 2n uint32 workspace.  Not bit-comparable with numpy's generator by
 * construction; tests check the distributions. */
int dis_augment(const float* im, const float* amb, const float* params, const long long* seed, unsigned* minmax_ws,
                float* out_im, float* out_amb, int n, int h, int w, void* stream);

/* ---------------------------------------------------------------- batch assembly ------------ */

/* Packed track files (depthinspace_amd/data/packed.py) -> the step's inputs, one launch.  raw: bs records on the DEVICE, record b at
 * raw + b * record_stride floats; a record holds, at the float offsets of `layout` (HOST struct; -1: the record has no such field),
 * im / ambient / disp / sgm_disp / primary_disp / pseudo_gt as (4, h, w), flow as (12, 2, h, w) in the pair order 01 02 03 10 12 13
 * 20 21 23 30 31 32, R (4, 3, 3), t (4, 3).  perm: (bs, tl) ints on the DEVICE, the frame order of every sample; every entry is masked
 * to 0..3 by the kernel.  `out` (HOST struct of DEVICE pointers; NULL: not wanted; im, ambient, disp, R, t are mandatory):
 *   out.X[i][b]            = record_b.X[perm[b][i]]                         X (tl, bs, 1, h, w); R (tl, bs, 3, 3); t (tl, bs, 3)
 *   out.flow[i * tl + j][b] = record_b.flow[pair(perm[b][i], perm[b][j])]   (tl * tl, bs, 2, h, w), pair(p, q) = 3p + q - (q > p);
 *                             the i == j planes (and those of a table with perm[b][i] == perm[b][j]) are zeros.
 * Every output element is written, nothing else is: safe in front of a hipGraph replay.  A streaming copy, 16 bytes per lane when
 * h * w, record_stride and the offsets are multiples of 4 floats and raw and the outputs are 16-byte aligned, 4 bytes otherwise.
 * Checks, in this order: a NULL raw / perm / layout / out / mandatory output -> DIS_ERR_NULL; bs, tl, h, w <= 0, tl > 4 or a field of
 * `layout` that does not lie inside [0, record_stride) -> DIS_ERR_BAD_SHAPE; an output whose field `layout` lacks ->
 * DIS_ERR_UNSUPPORTED.  The caller guarantees bs records behind raw and the output extents above. */
typedef struct DisTrackLayout {
  long im, ambient, disp, sgm_disp, primary_disp, pseudo_gt, flow, R, t;
} DisTrackLayout;
typedef struct DisTrackOut {
  float *im, *ambient, *disp, *sgm_disp, *primary_disp, *pseudo_gt, *flow, *R, *t;
} DisTrackOut;
int dis_assemble_tracks(const float* raw, long record_stride, const int* perm, const DisTrackLayout* layout, const DisTrackOut* out,
                        int bs, int tl, int h, int w, void* stream);

/* ---------------------------------------------------------------- track rendering ----------- */

/* A triangle-mesh scene seen by tl cameras -> what a track directory holds (depthinspace_amd/data/render.py writes it out): im,
 * ambient, disp and the exact rigid flow of every visible surface point for all ordered frame pairs, with occlusion and projector
 * shadows (csrc/render.hip).  The reference renders its tracks with connecting_the_dots' cyrender on ShapeNet meshes
 * (data/create_syn_data.py:147-257) and takes its flows from LiteFlowNet; neither is part of this library.
 * Image formation (the conventions of depthinspace_amd/synth.py, which the loss kernels assume):
 *   camera     X_c = R X_w + t; pixel (u, v) has the ray ((u - cx) / fx, (v - cy) / fy, 1); depth is the camera-frame z;
 *              disp = baseline fx / z.
 *   projector  rectified, centre (+baseline, 0, 0) in the camera frame; a point seen at (u, v) reads pattern(u - disp, v), bilinear
 *              with border clamp (dis_pattern_warp_fwd's lookup).
 *   primary    nearest intersection with t > 0 over ALL triangles (a triangle in front of any near distance is never clipped); on
 *              equal depth the lower triangle index wins.
 *   shadow     from the hit point to the projector centre: lit = 0 if any triangle other than the hit one meets that segment at a
 *              parameter in (eps, 1 - eps), eps = 1e-4 (0: the projector, 1: the hit point).  The origin is not offset: the hit
 *              triangle is excluded by index, a coplanar neighbour by eps.
 *   shading    face normal n flipped towards the viewer, c / p unit vectors from the point to the camera / projector centre,
 *              g the triangle's grey albedo, ka = 0.5, kd = 1.5:
 *                ambient = clip(g (ka + kd max(0, n.c)) / 2, 0, 1)
 *                P       = clip(g (ka + kd max(0, n.p)) / 2, 0, 1) pattern(u - disp, v) lit
 *                im      = clip(blend P + (1 - blend) ambient, 0, 1)          (no noise: dis_augment adds it at training time)
 *   flow       flow[i * tl + j](u, v) = pi_j(X_w) - (u, v) for the surface point visible in frame i, whether or not frame j sees
 *              it; the i == j planes are zeros.
 *   miss       disp = 0, flow 0, im = ambient = 0, lit = 0, tri_id = -1.
 * verts (nv, 3) world coordinates, faces (nf, 3) ints (an index outside [0, nv) is clamped, never followed), albedo (nf), R (tl, 3, 3),
 * t (tl, 3), pattern (h, w): DEVICE.  K4_host: {fx, fy, cx, cy}, HOST values read during the call.  `out`: HOST struct of DEVICE
 * pointers - im, ambient, disp (tl, 1, h, w) and flow (tl * tl, 2, h, w) are mandatory; tri_id (tl, h, w) ints and lit (tl, h, w) may
 * be NULL.  Every element of every output given is written.  workspace: dis_render_workspace(nv, nf, tl, h, w) BYTES (-1: an extent
 * is not supported), 16-byte aligned, no initialisation: per (frame, triangle) the camera-frame triangle, its plane and its screen
 * boxes; the candidate lists of the tiles live in LDS and never reach memory, so no scene can overflow them.
 * Two launches, no allocation, no synchronisation, no float atomics: capturable, and two calls on the same input give the same bits.
 * Checks, in this order: a NULL argument or mandatory output -> DIS_ERR_NULL; nv, nf, tl, h, w <= 0, tl > 4, nf > 2^20, nv > 2^24,
 * h or w > 8192 -> DIS_ERR_BAD_SHAPE; fx, fy or baseline not positive and finite, blend outside [0, 1], a misaligned workspace ->
 * DIS_ERR_UNSUPPORTED. */
typedef struct DisRenderOut {
  float *im, *ambient, *disp, *flow;
  int* tri_id;
  float* lit;
} DisRenderOut;
long dis_render_workspace(int nv, int nf, int tl, int h, int w);
int dis_render_track(const float* verts, const int* faces, const float* albedo, int nv, int nf, const float* R, const float* t,
                     const float* K4_host, float baseline, float blend, const float* pattern, const DisRenderOut* out, int tl, int h,
                     int w, void* workspace, void* stream);

/* ---------------------------------------------------------------- semi-global matching ------ */

/* Classical disparity of IR frames against the projector pattern (csrc/sgm.hip): what `--data_type real` training reads as sgm_disp
 * (dis_sgm_l1_fwd), and the baseline the networks are compared with.  Geometry as in "track rendering": pixel (u, v) sees
 * pattern(u - d, v); candidates d = 0 .. ndisp - 1.  Integer arithmetic up to the winning candidate; tests/sgm_ref.py restates it in
 * numpy and the kernels match it bit for bit.
 *   census    9 wide x 7 high window, replicate padding; the 62 neighbours in row-major order (dy, dx) = (-3, -4) .. (3, 4) without the
 *             centre; bit k (value 2^k) = neighbour < centre (strict, fp32, false for NaN).  Every frame, and the pattern once.
 *   cost      C(u, v, d) = popcount(cI(u, v) xor cP(u - d, v)) for u - d >= 0, else 64.  Never stored.
 *   paths     8 directions r; where p - r lies outside the image L_r(p, d) = C(p, d); elsewhere, m = min_k L_r(p - r, k),
 *             L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + p1, L_r(p - r, d + 1) + p1, m + p2) - m
 *             (no d +- 1 term outside [0, ndisp)).  S = sum_r L_r <= 8 (64 + 127) fits 16 bits.
 *   winner    d0 = argmin_d S (lowest d on ties), s0 = S(d0), s2 = min S over |d - d0| > 1.  Valid iff 1 <= d0 <= ndisp - 2,
 *             s2 (100 - uniq) > 100 s0, u - d0 >= 0 and |dR(u - d0, v) - d0| <= lr with dR(x, v) = argmin_d S(x + d, v, d) over
 *             x + d < w (lowest d on ties).  disp = d0 + (a - c) / (2 (a + c - 2 b)) for a, b, c = S(d0 - 1), S(d0), S(d0 + 1) in fp32
 *             when a + c - 2 b > 0, else d0; an invalid pixel gets 0.
 * im (n, h, w), pattern (h, w), disp (n, h, w): DEVICE; every element of disp is written.  Optional outputs (NULL: not wanted): d_int
 * (n, h, w) = d0 of every pixel, valid or not; vol = S as (n, h, w, ndisp) int16; census (n + 1, h, w) 64-bit words, the pattern's last.
 * workspace: dis_sgm_workspace(n, h, w, ndisp) BYTES (-1: unsupported extents or ndisp), 16-byte aligned, no initialisation.  Ten
 * launches, no allocation, no synchronisation, no atomics: capturable, and two calls on the same input give the same bits.
 * Checks, in this order: NULL im, pattern, disp or workspace -> DIS_ERR_NULL; n, h, w <= 0, h or w > 8192, (n + 1) h w >= 2^31 ->
 * DIS_ERR_BAD_SHAPE; ndisp not 64, 128 or 256, not 0 < p1 < p2 <= 127, uniq outside [0, 100), lr < 0, a misaligned workspace, vol or census
 * not 8-byte aligned -> DIS_ERR_UNSUPPORTED. */
long dis_sgm_workspace(int n, int h, int w, int ndisp);
int dis_sgm_disparity(const float* im, const float* pattern, float* disp, int* d_int, short* vol, long long* census, int n, int h, int w,
                      int ndisp, int p1, int p2, int uniq, int lr, void* workspace, void* stream);

/* ---------------------------------------------------------------- speckle filter ------------ */

/* Region-level post-filter of a disparity map (csrc/speckle.hip), the step classical pipelines run after the matcher's own checks: the
 * 4-connected components of similar disparity are labelled and the small ones are invalidated.  tests/speckle_ref.py restates it in
 * numpy and the kernels match it bit for bit.
 *   valid      0 < d < inf; NaN, +-inf, 0 and negative values are invalid.
 *   linked     two 4-neighbours of the same image, both valid, with fabsf(d_p - d_q) <= max_diff (the difference in fp32).
 *   component  a class of the transitive closure of `linked`: a ramp of max_diff per pixel is one component.
 *   out        the bits of disp where the pixel is valid and its component has MORE than max_size pixels, else 0.0f.  max_size 0 keeps
 *              every valid pixel; max_size >= h w empties the map.  Removing a component changes no other: the filter is idempotent.
 * disp, out (n, h, w): DEVICE; every element of out is written; out must not alias disp.  Optional outputs (NULL: not wanted): label
 * (n, h, w) int32 = y w + x of the component's first pixel in row order inside its image, -1 for an invalid pixel; size (n, h, w)
 * int32 = the pixels of the component, 0 for an invalid pixel.
 * workspace: dis_speckle_workspace(n, h, w) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation: every word that is
 * counted into is written first.  Four launches (three when the image is a single tile of 64 x 16), no allocation, no synchronisation:
 * capturable.  The only atomics are integer minima and integer adds whose results do not depend on the order: two calls on the same
 * input give the same bits.
 * Checks, in this order: NULL disp, out or workspace -> DIS_ERR_NULL; n, h, w <= 0, h or w > 8192, n h w >= 2^31 -> DIS_ERR_BAD_SHAPE;
 * max_size < 0, max_diff negative, NaN or infinite, a misaligned workspace -> DIS_ERR_UNSUPPORTED. */
long dis_speckle_workspace(int n, int h, int w);
int dis_speckle_filter(const float* disp, float* out, int* label, int* size, int n, int h, int w, int max_size, float max_diff,
                       void* workspace, void* stream);

/* ---------------------------------------------------------------- disparity densification --- */

/* The two stages classical pipelines run after the matcher and the speckle filter (csrc/densify.hip): holes inside one surface are
 * filled, then a median over the valid pixels removes sub-pixel noise.  tests/densify_ref.py restates it in numpy and the kernels match
 * it bit for bit: everything is selection and comparison.
 *   valid      0 < d < inf, the speckle filter's rule; NaN, +-inf, 0 and negative values are invalid.  Every invalid element of out is
 *              +0.0f.
 *   fill       max_gap 1 .. 32 (0: off).  From every invalid pixel, s = 1 .. max_gap steps in each of the 8 directions E, W, S, N, SE,
 *              SW, NE, NW inside the pixel's own image; the first valid pixel met gives the direction's value, a direction that leaves the
 *              image or meets none gives no value.  With m values in ascending order v[0] <= ... <= v[m - 1] the pixel becomes
 *              v[(m - 1) / 2] (the lower median) when m >= min_dirs (1 .. 8) and v[m - 1] - v[0] <= max_spread (one fp32 subtraction;
 *              max_spread in [0, FLT_MAX], FLT_MAX: no gate); otherwise it stays 0.  Only input values are read: a filled pixel is
 *              never a source.
 *   median     median_r 1 or 2 (0: off).  Every pixel that is valid after the fill becomes the lower median v[(k - 1) / 2] of the
 *              k >= 1 valid pixels of its (2 r + 1)^2 window after the fill, the window clipped to the image.  Only the fill's values
 *              are read.  Invalid pixels stay 0.
 * With max_gap = 0 and median_r = 0, out is disp with its invalid elements written as +0.0f.
 * disp, out (n, h, w): DEVICE; every element of out is written.  state (n, h, w) uint8, DEVICE, NULL: not wanted: 0 invalid, 1 valid in
 * the input, 2 filled; the median does not change it.  out and state must not overlap disp or each other.
 * workspace: dis_disp_densify_workspace(n, h, w) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation.  One launch per
 * stage that is on (one when neither is), no allocation, no synchronisation, no atomics: capturable, and two calls on the same input
 * give the same bits.
 * Checks, in this order, before anything is launched: NULL disp, out or workspace -> DIS_ERR_NULL; n, h, w <= 0, h or w > 8192,
 * n h w >= 2^31 -> DIS_ERR_BAD_SHAPE; max_gap outside 0 .. 32, min_dirs outside 1 .. 8, median_r outside 0 .. 2, max_spread negative,
 * NaN or infinite, a misaligned workspace, overlapping arrays -> DIS_ERR_UNSUPPORTED. */
long dis_disp_densify_workspace(int n, int h, int w);
int dis_disp_densify(const float* disp, float* out, unsigned char* state, int n, int h, int w, int max_gap, int min_dirs,
                     float max_spread, int median_r, void* workspace, void* stream);

/* ---------------------------------------------------------------- dense optical flow -------- */

/* flow_ij for every ordered pair of frames of a track (csrc/flow.hip): what the multi-frame stage reads from flow.npz, for tracks that
 * arrive without one.  A coarse-to-fine Horn-Schunck flow with warping, fp32; tests/flow_ref.py restates it in numpy, operand order
 * included.  Every border is replicate.  x is the column and channel 0, y the row and channel 1; flow_ij(p) is where pixel p of frame i
 * lies in frame j, minus p (the convention of synth.make_batch).
 *   normalise  per frame (I - mean) / max(std, 1e-6): its own population mean and standard deviation, accumulated in fp64 in a fixed
 *              order and rounded once to fp32.  A constant frame becomes zeros.
 *   pyramid    level 0 is the normalised frame; level k + 1 is level k under [1 4 6 4 1] / 16 over x, then over y - ((p[-2] + p[2]) +
 *              4 (p[-1] + p[1]) + 6 p[0]) / 16 - at the even rows and columns: ceil(h / 2) x ceil(w / 2).  A further level is built while
 *              min(h, w) >= 2 min_size at the coarsest.  One pyramid per frame, shared by its pairs.
 *   bilinear   img at (x, y), both clamped into the image: x0 = floor(x), x1 = min(x0 + 1, w - 1), fx = x - x0 (y alike),
 *              (I00 (1 - fx) + I01 fx) (1 - fy) + (I10 (1 - fx) + I11 fx) fy.
 *   per pair   (a, b) = frames (i, j), from the coarsest level to level 0, the flow starting at zero.  On entering a finer level
 *              u(x, y) = 2 bilinear(u_coarse, x / 2, y / 2), v alike.  Then `warps` times:
 *                bw = bilinear(b, x + u, y + v); m = (a + bw) / 2; Ix = (m(x + 1) - m(x - 1)) / 2, Iy alike; It = bw - a;
 *                den = (alpha^2 + Ix^2) + Iy^2; u0 = u, v0 = v; then `iters` Jacobi steps
 *                ub = ((l + r) + (t + b)) c6 + ((tl + tr) + (bl + br)) c12 over the 8 neighbours of u, c6 = fp32(1 / 6), c12 = fp32(1 / 12),
 *                vb alike; r = ((Ix (ub - u0) + Iy (vb - v0)) + It) / den; u = ub - Ix r; v = vb - Iy r.
 * frames (n, tl, h, w), flow (n, tl tl, 2, h, w): DEVICE; entry i tl + j of flow is flow_ij, the diagonal entries are zeros, every
 * element is written.  dbg: HOST struct, NULL in normal use; every pointer in it may be NULL.  With P = n tl (tl - 1) pairs in the order
 * track, i, j (j != i):
 *   pyr      the levels one after another, finest first: level k as (n, tl, h_k, w_k)
 *   warp     (4, P, h_l, w_l): bw, Ix, Iy, It of the last warp at level l = `level`
 *   levels   the flow when level k is left, one after another, finest first: level k as (P, 2, h_k, w_k)
 *   variant  0: the Jacobi steps run 8 per launch on a tile of (u, v) held in LDS; 1: one launch per step from memory - the same
 *            bits, kept for the rate comparison of scripts/flow_rate.py.
 * workspace: dis_flow_workspace(n, tl, h, w, min_size) BYTES (-1: unsupported), 16-byte aligned, no initialisation.  No allocation,
 * no synchronisation, no atomics: capturable, and two calls on the same input give the same bits.
 * Checks, in this order: NULL frames, flow or workspace -> DIS_ERR_NULL; n <= 0, tl outside 2 .. 4, h or w below 8 or above 8192,
 * n tl tl 2 h w >= 2^31 -> DIS_ERR_BAD_SHAPE; alpha not positive and finite, warps outside 1 .. 16, iters outside 1 .. 1024,
 * min_size < 4, a misaligned workspace, a variant other than 0 or 1, warp wanted at a level that does not exist ->
 * DIS_ERR_UNSUPPORTED.  (The size of the workspace is the caller's to guarantee; ops.dense_flow checks it.) */
typedef struct DisFlowDebug {
  float *pyr, *warp, *levels;
  int level, variant;
} DisFlowDebug;
long dis_flow_workspace(int n, int tl, int h, int w, int min_size);
int dis_dense_flow(const float* frames, float* flow, const DisFlowDebug* dbg, int n, int tl, int h, int w, float alpha, int warps,
                   int iters, int min_size, void* workspace, void* stream);

/* ---------------------------------------------------------------- track fusion -------------- */

/* The per-frame disparity maps of a track -> one point cloud in world coordinates, with a cross-view consistency measure that needs
 * no ground truth (csrc/fuse.hip).  Conventions of "track rendering": X_c = R X_w + t, the ray of pixel (u, v) is
 * ((u - cx) / fx, (v - cy) / fy, 1), disp = fx baseline / z.  fp32; tests/fuse_ref.py restates it in numpy, operand order included.
 * For track b, frame i, pixel (u, v):
 *   valid       disp is finite and > 0 (zero, negative, NaN and inf are holes).  z = (fx baseline) / disp, P = (z rx, z ry, z) with
 *               rx = (u - cx) / fx, ry = (v - cy) / fy; q = P - t_i; X_w = R_i^T q, each component (R[0][k] q0 + R[1][k] q1) + R[2][k] q2.
 *   projection  into frame j != i: X_j[k] = ((R_j[k][0] X_w0 + R_j[k][1] X_w1) + R_j[k][2] X_w2) + t_j[k];
 *               u_j = (fx X_j0) / X_j2 + cx, v_j = (fy X_j1) / X_j2 + cy.
 *   seen in j   the pixel is valid, X_j2 > 0, 0 <= u_j <= w - 1, 0 <= v_j <= h - 1, and the four pixels of the bilinear cell
 *               x0 = min(floor(u_j), w - 2), y0 = min(floor(v_j), h - 2) are valid in frame j.
 *   z_s         frame j's DEPTH (fx baseline) / disp interpolated over the cell, ax = u_j - x0, ay = v_j - y0:
 *               (z00 (1 - ax) + z01 ax) (1 - ay) + (z10 (1 - ax) + z11 ax) ay.
 *   rel_ij      |z_s - X_j2| / X_j2.  consistent with j: seen and rel_ij <= tol.
 *   views       1 + the number of consistent j; 0 for an invalid pixel.  seen: the number of j that see the pixel.
 *   resid       the mean of rel_ij over the seen j (summed in ascending j), 0 with none.
 *   point       the mean of X_w and of one sample point per consistent j, R_j^T (X_j (z_s / X_j2) - t_j): the point on camera j's ray
 *               at the sampled depth.  Summed from X_w in ascending j, divided by views.  Zeros for an invalid pixel.
 *   normal      c = (P(u + 1, v) - P(u - 1, v)) x (P(u, v + 1) - P(u, v - 1)) in camera i, divided by its length
 *               sqrt((c0 c0 + c1 c1) + c2 c2), negated when (n0 P0 + n1 P1) + n2 P2 > 0 (it faces the camera), rotated by R_i^T.  The zero
 *               vector where the pixel or one of the four neighbours is invalid or outside the image, or the length is zero or not
 *               finite.
 *   value       the pixel of the optional plane carried along (the ambient image); 0 without one.
 *   keep        valid, views >= min_views, and no j < i is consistent: the lowest-index frame that sees a surface owns it.  That removes
 *               the tl-fold duplication by a per-pixel rule with no "already used" marking; it leans on consistency being nearly
 *               symmetric (if pixel p of frame i is consistent with frame j, the surface's pixel in frame j is almost always consistent
 *               with frame i; where it is not - at the rim of the tolerance, next to holes and image borders - a surface point can be
 *               kept twice or not at all).
 * Packed output: the kept pixels in ascending order of src = ((b tl + i) h + v) w + u; track b's records start at the sum of the counts
 * before it.  If more pixels are kept than `cap`, the first `cap` are written; `count` still holds the true numbers; nothing is
 * written past `cap`, and records beyond the sum of the counts are not written at all.
 * disp (n, tl, h, w), R (n, tl, 3, 3), t (n, tl, 3), value (n, tl, h, w) or NULL: DEVICE.  K4_host = {fx, fy, cx, cy}: HOST.
 * out: HOST struct of DEVICE pointers.  xyz (cap, 3), normal (cap, 3), value (cap) fp32, src (cap) int32 - these four may be NULL
 * when cap == 0; count (n) int32; the dense maps views, seen, keep (n, tl, h, w) uint8 and resid (n, tl, h, w) fp32 - all written in
 * full; point, dnormal (n, tl, 3, h, w) fp32 planar, NULL: kept in the workspace.
 * Three launches: the check kernel (one lane per pixel; the kept count of every 256-pixel block by 64-bit ballots), an exclusive scan of
 * the block counts by one workgroup (which also forms `count`), the scatter (block offset + rank inside the block).  The hand-off
 * between them is the launch boundary alone: no atomics, no flags polled between workgroups, so the result does not depend on where
 * workgroups run and two calls give the same bits.  No allocation, no synchronisation: capturable.
 * workspace: dis_fuse_workspace(n, tl, h, w) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation.
 * Checks, in this order, all before any launch: NULL disp, R, t, K4_host, out, workspace, count or a dense map other than point and
 * dnormal, a NULL packed array with cap > 0 -> DIS_ERR_NULL; n < 1, tl outside 2 .. 4, h or w outside 2 .. 8192, n tl h w >= 2^31 ->
 * DIS_ERR_BAD_SHAPE; tol not in (0, 1), min_views outside 1 .. tl, fx, fy or baseline not positive and finite, cx or cy not finite,
 * cap < 0, workspace_bytes below dis_fuse_workspace(...), a misaligned workspace -> DIS_ERR_UNSUPPORTED. */
typedef struct DisFuseOut {
  float *xyz, *normal, *value;
  int *src, *count;
  unsigned char *views, *seen, *keep;
  float *resid, *point, *dnormal;
} DisFuseOut;
long dis_fuse_workspace(int n, int tl, int h, int w);
int dis_fuse_track(const float* disp, const float* R, const float* t, const float* K4_host, float baseline, const float* value,
                   float tol, int min_views, int cap, const DisFuseOut* out, int n, int tl, int h, int w, void* workspace,
                   long workspace_bytes, void* stream);

/* ---------------------------------------------------------------- track poses --------------- */

/* The relative camera pose of every ordered pair of frames of a track, from the per-frame disparities and the pairwise flows
 * (csrc/pose.hip): what gives R and t to a track that arrives with images only.  Conventions of "track rendering" and "track fusion":
 * X_c = R X_w + t, the ray of pixel (u, v) is ((u - cx) / fx, (v - cy) / fy, 1), disp = fx baseline / z; flow_ij(p) is where pixel p of
 * frame i lies in frame j, minus p.  For track b and the ordered pair (i, j), i != j, the estimate is the transform from camera-i to
 * camera-j coordinates, X_j = R_ij X_i + t_ij (R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i): `iters` Gauss-Newton steps, from the identity,
 * on the residual in (u, v, disparity) of frame j, in pixels.  tests/pose_ref.py restates it in numpy, operand order included.  With
 * fb = fx baseline (formed in fp32 on the host) and s2 = scale scale (alike), every per-pixel operation below is one fp32 operation:
 *   valid      disp is finite and > 0.  z = fb / disp, P = (z rx, z ry, z) with rx = (u - cx) / fx, ry = (v - cy) / fy.
 *   target     in frame j, the same in every pass: uj = u + flow.x, vj = v + flow.y.  The pixel is matched iff it is valid in frame i,
 *              0 <= uj <= w - 1, 0 <= vj <= h - 1 (comparisons are false for NaN) and the four pixels of the cell x0 = min(floor(uj), w - 2),
 *              y0 = min(floor(vj), h - 2) are valid in frame j.  ds is frame j's DISPARITY (not the depth: the disparity of a plane is affine
 *              in the pixel, so the sample is exact there) over the cell, ax = uj - x0, ay = vj - y0:
 *              ds = (d00 (1 - ax) + d01 ax) (1 - ay) + (d10 (1 - ax) + d11 ax) ay.
 *              A pixel that is not matched adds nothing (a select, never 0 x).
 *   state      (R, t) per pair in fp64, set to the identity by the call itself.  Pass k = 0 .. iters uses its fp32 rounding:
 *              X[c] = ((R[c][0] P0 + R[c][1] P1) + R[c][2] P2) + t[c].  The pixel is used iff it is matched and X2 > 0.
 *   residual   iz = 1 / X2, px = X0 iz, py = X1 iz; e = ((fx px + cx) - uj, (fy py + cy) - vj, fb iz - ds);
 *              r2 = (e0 e0 + e1 e1) + e2 e2; g = 1 / (1 + r2 / s2); the weight is 1 in pass 0 and g g afterwards (from the identity every
 *              residual exceeds `scale`; the first step is the unweighted one).
 *   Jacobian   of e under a left perturbation X' = X + omega x X + nu.  a = fx iz, b = fy iz, c = fb iz, g0 = -(a px), g1 = -(b py),
 *              g2 = -(c iz); the rows over (omega, nu), their structural zeros never multiplied:
 *                J_0 = (g0 X1,         a X2 - g0 X0,   -(a X1),   a, 0, g0)
 *                J_1 = (g1 X1 - b X2,  -(g1 X0),       b X0,      0, b, g1)
 *                J_2 = (g2 X1,         -(g2 X0),       0,         0, 0, g2)
 *   sums       30 per pair and pass: H_pq = sum (weight J_r[p]) J_r[q] for p <= q, g_p = sum (weight J_r[p]) e_r, S_w = sum weight,
 *              S_c = sum weight r2, n = the number of used pixels.  Every term is formed in fp32, converted to fp64 and added in fp64
 *              (so the order of the additions changes the result far below one fp32 ulp).
 *   solve      fp64, one workgroup per pair.  The pair fails if n < min_corr, or if a pivot of the Cholesky factorisation of
 *              H + damping diag(H) is not > 0 or not finite; a failed pair keeps the state of its last good step (the identity if there
 *              is none) and takes no further steps.  Else delta = -(H + damping diag(H))^-1 g, omega = delta[0:3], nu = delta[3:6],
 *              th2 = omega . omega, dR = I + A [omega]x + B [omega]x^2 with A = sin th / th, B = (1 - cos th) / th2 (A = 1, B = 1 / 2 when
 *              th2 < 1e-16), R <- dR R, t <- dR t + nu.
 *   closing    after the last step one more pass at the final state, with the weight g g, yields the statistics.
 * disp (n, tl, h, w), flow (n, tl tl, 2, h, w) - the output layout of dis_dense_flow; the diagonal entries are not read - : DEVICE.
 * K4_host = {fx, fy, cx, cy}: HOST.  Outputs, DEVICE, every element written: R_pair (n, tl, tl, 3, 3), t_pair (n, tl, tl, 3),
 * stats (n, tl, tl, 4) = {n, S_w / n, sqrt(S_c / S_w), status} of the closing pass, fp32; status 1: every step was taken, 0: failed; the
 * ratios are 0 when the pair has no used pixel.  The diagonal is the identity, zeros and {0, 0, 0, 1}.
 * iters + 1 accumulate launches (each lane a grid-stride range of a pair's pixels - the target is recomputed in every pass, there is no
 * per-pixel workspace -, a sum over the wave, over the workgroup's waves through LDS, one record of partial sums per workgroup) and
 * iters + 1 solve launches (the records of a pair added in ascending workgroup order).  The hand-off between them is the launch
 * boundary alone: no atomics, so two calls give the same bits.  No allocation, no synchronisation: capturable.
 * workspace: dis_pose_workspace(n, tl, h, w) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation.
 * Checks, in this order, all before any launch: a NULL pointer -> DIS_ERR_NULL; n < 1, tl outside 2 .. 4, h or w outside 2 .. 8192,
 * n tl tl 2 h w >= 2^31 -> DIS_ERR_BAD_SHAPE; iters outside 1 .. 64, scale not positive and finite, damping negative or not finite,
 * min_corr < 6, fx, fy or baseline not positive and finite, cx or cy not finite, workspace_bytes below dis_pose_workspace(...), a
 * misaligned workspace -> DIS_ERR_UNSUPPORTED. */
long dis_pose_workspace(int n, int tl, int h, int w);
int dis_track_poses(const float* disp, const float* flow, const float* K4_host, float baseline, int iters, float scale, float damping,
                    int min_corr, float* R_pair, float* t_pair, float* stats, int n, int tl, int h, int w, void* workspace,
                    long workspace_bytes, void* stream);

/* dis_refine_track_poses: the second stage.  One pose per frame of a track, frame 0 fixed, refined at once on the residuals of every used
 * ordered pair - the per-pixel expressions of dis_track_poses above, unchanged: valid, target, matched, used, residual, Jacobian and the
 * 30 sums - so that the pairs that dis_track_poses estimates independently hold each other.  tests/pose_joint_ref.py restates what is
 * added here in numpy, operand order included.
 *   state      (R_k, t_k) per frame in fp64, X_c = R_k X_w + t_k, converted from R_init, t_init by the call itself.  Frame 0 is never
 *              moved: its output equals its input bit for bit.
 *   pair       pass k = 0 .. iters forms, for every used pair (i, j), in fp64
 *                R_ij[r][c] = (R_j[r][0] R_i[c][0] + R_j[r][1] R_i[c][1]) + R_j[r][2] R_i[c][2],
 *                t_ij[r] = t_j[r] - ((R_ij[r][0] t_i[0] + R_ij[r][1] t_i[1]) + R_ij[r][2] t_i[2]);
 *              their fp32 rounding is the state of the per-pixel expressions.  Every pass, the first included, uses the weight g g (the
 *              refinement starts from an estimate: there is no unweighted pass).  pair_use[b][i][j] != 0: the pair is used; NULL:
 *              every pair off the diagonal; the diagonal is ignored.  The flows of a pair that is not used are not read.
 *   contribute a pair contributes to a pass iff it is used and its n >= min_corr in that pass.
 *   assembly   fp64.  With Ad_ij = [[R_ij, 0], [[t_ij]x R_ij, R_ij]] acting on (omega, nu) - ([t]x R)[r][c] = t[r+1] R[r+2][c] -
 *              t[r+2] R[r+1][c], indices mod 3, from the fp64 R_ij, t_ij - a left perturbation xi_k of every frame perturbs the pair by
 *              xi_j - Ad_ij xi_i.  Per pair M = H Ad, N = Ad^T M, q = Ad^T g, every element the sum over k = 0 .. 5 in this order from the
 *              first product (the structural zeros of Ad are multiplied); then, over the contributing pairs in ascending (i, j), from
 *              zero: A[j,j] += H, A[i,i] += N, A[j,i] -= M, A[i,j] -= M^T, b[j] += g, b[i] -= q.  The rows and columns of frame 0 are
 *              dropped: the order is 6 (tl - 1).
 *   solve      Cholesky of A + damping diag(A), column by column as for a pair; L y = -b with k ascending, L^T delta = y with k
 *              descending, an unknown being its row's sum times 1 / L_kk (formed once per column); frame k >= 1 takes delta[6 (k - 1) .. 6 k) = (omega, nu) through the update of dis_track_poses (dR from omega,
 *              R_k <- dR R_k, t_k <- dR t_k + nu).
 *   failure    a track fails when a pivot is not > 0 or not finite - which a frame that no contributing pair touches gives, and so does a
 *              pass without any contributing pair.  A failed track keeps the state of its last good step (the init if there is none)
 *              and takes no further steps.
 *   closing    after the last step one more pass at the final state yields the statistics.
 * disp, flow, K4_host, baseline: as in dis_track_poses.  R_init (n, tl, 3, 3), t_init (n, tl, 3) fp32, pair_use (n, tl, tl) uint8 or NULL:
 * DEVICE.  Outputs, DEVICE, every element written, fp32: R (n, tl, 3, 3), t (n, tl, 3); pair_stats (n, tl, tl, 4) = {n, S_w / n,
 * sqrt(S_c / S_w), contributed} of the closing pass, zeros for a pair that is not used, {0, 0, 0, 1} on the diagonal; track_stats (n, 4) =
 * {contributing pairs, sum n, sqrt(sum S_c / sum S_w), status}, the sums over the contributing pairs of the closing pass in ascending
 * (i, j); status 1: every step was taken, 0: failed.  A ratio is 0 where a denominator is 0.
 * iters + 1 accumulate launches (the grid and the reduction of dis_track_poses; the pair's state is composed inside the kernel) and
 * iters + 1 solve launches (a workgroup per track: the records of a pair added in ascending workgroup order, the system assembled,
 * factored and solved in LDS): 2 (iters + 1) launches.  The hand-off between them is the launch boundary alone: no atomics, no flags
 * polled between workgroups, so two calls give the same bits.  No allocation, no synchronisation: capturable.
 * workspace: dis_pose_joint_workspace(n, tl, h, w) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation.
 * Checks, in this order, all before any launch: a NULL pointer other than pair_use -> DIS_ERR_NULL; n < 1, tl outside 2 .. 4, h or w
 * outside 2 .. 8192, n tl tl 2 h w >= 2^31 -> DIS_ERR_BAD_SHAPE; iters outside 1 .. 64, scale not positive and finite, damping negative or
 * not finite, min_corr < 6, fx, fy or baseline not positive and finite, cx or cy not finite, workspace_bytes below
 * dis_pose_joint_workspace(...), a misaligned workspace -> DIS_ERR_UNSUPPORTED. */
long dis_pose_joint_workspace(int n, int tl, int h, int w);
int dis_refine_track_poses(const float* disp, const float* flow, const float* K4_host, float baseline, const float* R_init,
                           const float* t_init, const unsigned char* pair_use, int iters, float scale, float damping, int min_corr,
                           float* R, float* t, float* pair_stats, float* track_stats, int n, int tl, int h, int w, void* workspace,
                           long workspace_bytes, void* stream);

/* ---------------------------------------------------------------- disparity alignment ------- */

/* The relative camera pose of every ordered pair of frames of a track from its disparity maps ALONE (csrc/disp_align.hip): direct
 * coarse-to-fine alignment of frame i's disparity map onto frame j's, Gauss-Newton on the residual in disparity, from the identity.  No
 * flow is read: on flat-shaded surfaces an image-based flow finds nothing, the disparity maps carry the geometry.  The residual is in
 * disparity (pixels), not in metres, so that a disparity noise weighs every depth alike.  Conventions and outputs are those of
 * dis_track_poses: X_j = R_ij X_i + t_ij.  tests/disp_align_ref.py restates it in numpy, operand order included.  fb = fx baseline,
 * s2 = scale scale, jump2 = 2 jump are formed in fp32 on the host; every per-pixel operation below is one fp32 operation.
 *   valid      a disparity that is finite and > 0.
 *   pyramid    per frame.  Level 0 is the input; level l + 1 has floor(h_l / 2) x floor(w_l / 2) cells (an odd last row or column is
 *              dropped).  With a[0 .. 4) the block's disparities in the order 00, 01, 10, 11 (row, column): m = the largest valid one
 *              (0 with none); a cell is the sum of the valid a[k] >= 0.9f m, added in that order from 0, divided by their number - the
 *              nearer surface wins, nothing is averaged across a depth edge -, 0 with none.  Disparities stay in full-resolution pixels
 *              on every level: z = fb / d everywhere.  Intrinsics (host, fp32): fx_l = fx_{l-1} / 2, cx_l = (cx_{l-1} - 0.5) / 2, y alike.
 *   maps       per frame and level, one float4 per pixel {D, Dx, Dy, good}: D the disparity, Dx = 0.5 (d(x + 1) - d(x - 1)),
 *              Dy = 0.5 (d(y + 1) - d(y - 1)); good (1.0) iff the pixel has its four neighbours inside the image, all five are valid,
 *              |Dx| < jump D and |Dy| < jump D; all four are 0 where not good.
 *   state      (R, t) per pair in fp64, set to the identity by the call itself and carried across the levels unchanged.  A pass at
 *              level l uses its fp32 rounding and the level's intrinsics.  For pixel (u, v) of frame i's level l with a valid d:
 *              z = fb / d, P = (z ((u - cx_l) / fx_l), z ((v - cy_l) / fy_l), z); Y[c] = ((R[c][0] P0 + R[c][1] P1) + R[c][2] P2) + t[c];
 *              skipped unless Y2 > 0.  iz = 1 / Y2, px = Y0 iz, py = Y1 iz, u' = fx_l px + cx_l, v' = fy_l py + cy_l.
 *   target     us = u' + 2^-6, vs = v' + 2^-6; skipped unless 0 <= us < w_l - 1 and 0 <= vs < h_l - 1 (false for NaN); x0 = floor(us),
 *              y0 = floor(vs); skipped unless the maps of frame j are good at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).
 *              ax = u' - x0, ay = v' - y0 (>= -2^-6: the cell's own interpolant, continued), bx = 1 - ax, by = 1 - ay; D, Gx, Gy are
 *              (m00 bx + m01 ax) by + (m10 bx + m11 ax) ay of the three maps.  (The 2^-6: at the identity every target lies on an
 *              integer up to rounding; with the cells' boundary there the last bit would choose the cell, and with it the four taps.)
 *   residual   pred = fb iz, e = D - pred; skipped unless |e| < jump2 pred.
 *   Jacobian   g0 = Gx (fx_l iz), g1 = Gy (fy_l iz), g2 = pred iz - (g0 Y0 + g1 Y1) iz;
 *              J = (Y1 g2 - Y2 g1, Y2 g0 - Y0 g2, Y0 g1 - Y1 g0, g0, g1, g2) over (omega, nu) of a left perturbation.
 *   weight     1 in the first pass of the coarsest level, else q q with q = 1 / (1 + (e e) / s2).
 *   sums       the 30 of dis_track_poses with the one row J: H_pq = sum (weight J[p]) J[q], g_p = sum (weight J[p]) e, S_w = sum weight,
 *              S_c = sum weight (e e), n; every term formed in fp32 and added in fp64.
 *   schedule   iters_host[l] steps at level l (iters_host: HOST, `levels` ints, finest first), the coarsest level first; the step and
 *              its failure are those of dis_track_poses (n < min_corr, or a pivot that is not > 0 and finite: the pair keeps its last
 *              good state and takes no further step at any level).  One closing pass at level 0, weighted, gives the statistics.
 * disp (n, tl, h, w): DEVICE.  K4_host = {fx, fy, cx, cy}: HOST.  Outputs, DEVICE, every element written: R_pair (n, tl, tl, 3, 3),
 * t_pair (n, tl, tl, 3), stats (n, tl, tl, 4) = {n, S_w / n, sqrt(S_c / S_w), status} of the closing pass, as dis_track_poses writes them;
 * the diagonal is the identity, zeros and {0, 0, 0, 1}.
 * dbg: HOST struct, NULL in normal use; every pointer in it may be NULL.  pyr: the levels 1 .. levels - 1 one after another, level l
 * as (n, tl, h_l, w_l); maps: (n, tl, h_l, w_l, 4) of level l = `level`; sums: (passes, n, tl, tl, 30) fp64, passes = sum iters + 1, zeros
 * on the diagonal.
 * Launches: one per level above 0 for the pyramid, one per level for the maps (a lane per cell, every frame in the grid); then one
 * accumulate launch (a wave per 8 x 8 patch of frame i, 2 x 2 waves per workgroup, the workgroups of a pair taking its 16 x 16 tiles in
 * turn; the reduction of dis_track_poses) and one solve launch per pass, every ordered pair of every track in each grid.  The hand-off
 * is the launch boundary alone: no atomics, no flags, so two calls give the same bits.  No allocation, no synchronisation: capturable.
 * workspace: dis_disp_align_workspace(n, tl, h, w, levels) BYTES (-1: unsupported extents or levels), 16-byte aligned, no initialisation.
 * Checks, in this order, all before any launch: a NULL pointer other than dbg -> DIS_ERR_NULL; n < 1, tl outside 2 .. 4, h or w outside
 * 2 .. 8192, n tl tl 2 h w >= 2^31 -> DIS_ERR_BAD_SHAPE; levels outside 1 .. 6, a coarsest level below 8 x 8, an iters_host[l] outside
 * 0 .. 64, their sum 0, scale not positive and finite, damping negative or not finite, min_corr < 6, jump outside (0, 1), fx, fy or
 * baseline not positive and finite, cx or cy not finite, workspace_bytes below dis_disp_align_workspace(...), a misaligned workspace,
 * maps wanted at a level that does not exist -> DIS_ERR_UNSUPPORTED. */
typedef struct DisDispAlignDebug {
  float *pyr, *maps;
  double* sums;
  int level;
} DisDispAlignDebug;
long dis_disp_align_workspace(int n, int tl, int h, int w, int levels);
int dis_disp_align_poses(const float* disp, const float* K4_host, float baseline, int levels, const int* iters_host, float scale,
                         float damping, int min_corr, float jump, float* R_pair, float* t_pair, float* stats,
                         const DisDispAlignDebug* dbg, int n, int tl, int h, int w, void* workspace, long workspace_bytes, void* stream);

/* dis_rigid_flow: the flow that disparities and poses imply (csrc/disp_align.hip) - flow.npz without an image-based estimator, for a
 * static scene.  For track b, the ordered pair (i, j), i != j, and pixel (u, v) of frame i with a valid d (fp32, tests/disp_align_ref.py):
 * P as in "track fusion" (z = fb / d, P = (z ((u - cx) / fx), z ((v - cy) / fy), z)), X_w = R_i^T (P - t_i), Y = R_j X_w + t_j in the
 * operand orders given there; with Y2 > 0: u_j = (fx Y0) / Y2 + cx, v_j = (fy Y1) / Y2 + cy, flow = (u_j - u, v_j - v).  An invalid d
 * or Y2 <= 0 writes zeros, as does the diagonal.  visible (optional, NULL: not wanted): 1 iff the flow was written,
 * 0 <= u_j + 0.5 < w, 0 <= v_j + 0.5 < h, frame j's disparity d_j at (floor(u_j + 0.5), floor(v_j + 0.5)) is valid and
 * |d_j - pred| <= tol pred with pred = fb / Y2; 0 on the diagonal.
 * disp (n, tl, h, w), R (n, tl, 3, 3), t (n, tl, 3) (X_c = R X_w + t): DEVICE.  K4_host: HOST.  flow (n, tl tl, 2, h, w) - the layout of
 * dis_dense_flow -, visible (n, tl tl, h, w) uint8: DEVICE, every element written.  One launch, a lane per pixel of a pair; capturable.
 * Checks, in this order: NULL disp, R, t, K4_host or flow -> DIS_ERR_NULL; the extents of dis_track_poses -> DIS_ERR_BAD_SHAPE; tol not
 * in (0, 1), fx, fy or baseline not positive and finite, cx or cy not finite -> DIS_ERR_UNSUPPORTED. */
int dis_rigid_flow(const float* disp, const float* R, const float* t, const float* K4_host, float baseline, float tol, float* flow,
                   unsigned char* visible, int n, int tl, int h, int w, void* stream);

/* ---------------------------------------------------------------- volumetric fusion --------- */

/* The per-frame disparity maps of ONE track -> a truncated signed distance volume on a regular lattice, and the volume -> an indexed
 * triangle mesh by naive surface nets (csrc/tsdf.hip), or cast back into per-pixel maps of any camera (csrc/raycast.hip).  Conventions of "track rendering" and "track fusion": X_c = R X_w + t,
 * disp = fx baseline / z, a disparity is valid when it is finite and > 0.  fp32; tests/tsdf_ref.py restates both in numpy, operand
 * order included.  One track per call (a volume can fill the device); no atomics: two calls give the same bits.
 *
 * dis_tsdf_integrate.  fb = fx baseline is formed in fp32 on the host.  For lattice point (i, j, k), 0 <= i < nx and so on,
 *   X = (ox + float(i) voxel, oy + float(j) voxel, oz + float(k) voxel), formed from the indices for every point on its own.
 * For the frames f = 0 .. tl - 1, in this order:
 *   Xc_r = ((R_f[r][0] X0 + R_f[r][1] X1) + R_f[r][2] X2) + t_f[r]; z = Xc_2.  The frame is skipped unless z > 0.
 *   pu = floor((fx (Xc_0 / z) + cx) + 0.5), pv = floor((fy (Xc_1 / z) + cy) + 0.5): the NEAREST pixel (a bilinear depth across a
 *   silhouette would invent surface).  The frame is skipped unless 0 <= pu <= w - 1 and 0 <= pv <= h - 1, compared as floats before
 *   any conversion to an integer (false for NaN).
 *   d = disp[f][pv][pu]; skipped unless valid.  depth = fb / d, sdf = depth - z.  Skipped if sdf < -trunc (behind the surface).
 *   Otherwise acc = acc + min(sdf / trunc, 1), weight = weight + 1, and where sdf <= trunc also vsum = vsum + value[f][pv][pu],
 *   vcnt = vcnt + 1.
 * tsdf = acc / float(weight), or 1 where weight is 0; vvalue = vsum / float(vcnt), or 0 where vcnt is 0 (and everywhere without a
 * value plane).  Every frame weighs 1.
 * disp (tl, h, w), R (tl, 3, 3), t (tl, 3), value (tl, h, w) or NULL: DEVICE.  K4_host = {fx, fy, cx, cy}, origin3_host = {ox, oy, oz}:
 * HOST.  Outputs, DEVICE, every element written: tsdf (nz, ny, nx) fp32, weight (nz, ny, nx) uint8, vvalue (nz, ny, nx) fp32.
 * One launch, one lane per lattice point, the lanes along x; no workspace, no allocation, no synchronisation: capturable.
 * Checks, in this order, all before the launch: a NULL pointer other than value -> DIS_ERR_NULL; tl outside 1 .. 4, h or w outside
 * 2 .. 8192, nx, ny or nz outside 2 .. 1024 -> DIS_ERR_BAD_SHAPE; voxel, trunc, fx, fy, baseline or fx baseline not positive and
 * finite, cx, cy or a component of the origin not finite -> DIS_ERR_UNSUPPORTED. */
int dis_tsdf_integrate(const float* disp, const float* R, const float* t, const float* K4_host, float baseline, const float* value,
                       const float* origin3_host, float voxel, float trunc, float* tsdf, unsigned char* weight, float* vvalue, int tl,
                       int h, int w, int nx, int ny, int nz, void* stream);

/* dis_tsdf_mesh: naive surface nets (one vertex per cell the surface passes through, one quad per lattice edge it crosses: no case
 * table, shared vertices by construction).  neg(p) = tsdf[p] < 0.
 *   cell      (i, j, k), i <= nx - 2 and so on, has the corners c = 0 .. 7 at the offsets (c & 1, c >> 1 & 1, c >> 2).  It is active when
 *             all eight corner weights are >= min_weight and the eight neg bits are neither all set nor all clear.
 *   edges     the 12 cell edges in the order: axis a = x, y, z; inside an axis (p, q) = (0, 0), (0, 1), (1, 0), (1, 1), p the offset
 *             along axis a + 1 and q along a + 2 (cyclic).  lo is the corner with offset 0 along a, hi the one with offset 1;
 *             fa = tsdf[lo], fb = tsdf[hi].  An edge with neg(lo) != neg(hi) adds the point with fa / (fa - fb) along a, float(p) and
 *             float(q) along the others, to three running sums (sum = sum + coordinate, from 0, in edge order) and 1 to their number.
 *   vertex    local = sum / float(number); position o + (float(index) + local) voxel per axis.  normal: g_a = the sum of (fb - fa) over
 *             the four edges of axis a (from the first difference, in edge order), divided by sqrt((g0 g0 + g1 g1) + g2 g2) - towards
 *             positive tsdf, which is free space -, zeros when that length is zero or not finite.  value: the eight corner vvalues
 *             added in corner order, from corner 0, divided by 8.  views: the smallest corner weight.
 *   ids       vertex ids are the ranks of the active cells in the linear order (k, j, i); cell = (k (ny - 1) + j) (nx - 1) + i.
 *   faces     every lattice point p and axis a (x, y, z) with p_a <= n_a - 2 and 1 <= p_b <= n_b - 2 on the two other axes yields a quad
 *             when neg(p) != neg(p + e_a) and the four cells at the offsets (-1, -1), (0, -1), (0, 0), (-1, 0) along (a + 1, a + 2) - and
 *             p_a along a - are all active.  Their vertex ids in this order are (q0, q1, q2, q3); the order is reversed when tsdf[p] >= 0
 *             (not neg(p)).  Two triangles (q0, q1, q2), (q0, q2, q3), so that the face normals point to free space.  Faces are ordered
 *             by the linear index of p, then by axis.
 * tsdf, weight, vvalue (nz, ny, nx): DEVICE.  origin3_host: HOST.  out: HOST struct of DEVICE pointers.  xyz (vcap, 3), normal (vcap, 3),
 * value (vcap) fp32, views (vcap) uint8, cell (vcap) int32 ascending - these five may be NULL when vcap == 0; faces (fcap, 3) int32, may be
 * NULL when fcap == 0; count (2) int32 = the true numbers of vertices and of triangles, whatever the caps (int32: more than 2^31 - 1
 * triangles are not counted right); vid (nz - 1, ny - 1, nx - 1) int32, the dense vertex ids, -1 where the cell is inactive, NULL: kept in
 * the workspace.  Rows at or beyond a cap are not written, nor is a triangle that names a vertex >= vcap (it is still counted); rows at
 * and beyond the counts are not written at all.
 * Five launches: flags (the eight-corner stencil of a 256-point block staged in LDS as four linear rows of 257; the active count of
 * every block by 64-bit ballots), quads (the quad count of every block), one scan of both count arrays (a workgroup each, which also
 * forms `count`), vertices (block offset + rank inside the block), faces.  The hand-off between them is the launch boundary alone: no
 * atomics, no flags polled between workgroups.  No allocation, no synchronisation: capturable.
 * workspace: dis_tsdf_mesh_workspace(nx, ny, nz) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation.
 * Checks, in this order, all before any launch: NULL tsdf, weight, vvalue, origin3_host, out, workspace or count, a NULL vertex array
 * with vcap > 0, NULL faces with fcap > 0 -> DIS_ERR_NULL; nx, ny or nz outside 2 .. 1024 -> DIS_ERR_BAD_SHAPE; voxel not positive and
 * finite, a component of the origin not finite, min_weight outside 1 .. 4 (the longest track), vcap or fcap < 0, workspace_bytes below
 * dis_tsdf_mesh_workspace(...), a misaligned workspace -> DIS_ERR_UNSUPPORTED. */
typedef struct DisTsdfMeshOut {
  float *xyz, *normal, *value;
  unsigned char* views;
  int *cell, *faces, *count, *vid;
} DisTsdfMeshOut;
long dis_tsdf_mesh_workspace(int nx, int ny, int nz);
int dis_tsdf_mesh(const float* tsdf, const unsigned char* weight, const float* vvalue, const float* origin3_host, float voxel,
                  int min_weight, int vcap, int fcap, const DisTsdfMeshOut* out, int nx, int ny, int nz, void* workspace,
                  long workspace_bytes, void* stream);

/* dis_tsdf_raycast: the volume read back in a camera's view (csrc/raycast.hip): per pixel of nv views - they need not be the track's
 * frames - the first crossing of the trilinear tsdf from free space into the surface along the pixel's ray.  tests/raycast_ref.py
 * restates it in numpy, operand order included.  For the pixel (u, v) of view f, R = R_f, t = t_f:
 *   ray       dc = ((float(u) - cx) / fx, (float(v) - cy) / fy, 1); the camera centre o_k = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2), the
 *             direction d_k = (R[0][k] dc0 + R[1][k] dc1) + R[2][k]: the ray is parameterised by the camera depth z.
 *   samples   anchored at the camera: z_n = float(n) step for n = 1 .. 2^24 - 1, formed from n for every sample on its own.  Lattice
 *             coordinate g_a = ((o_a + z_n d_a) - origin_a) / voxel.  The sample is inside when 0 <= g_a < float(n_a - 1) on the three
 *             axes, compared as floats (false for NaN); then i_a = floor(g_a), f_a = g_a - float(i_a).  It is valid when it is inside and
 *             the eight corner weights of cell (i_x, i_y, i_z) are all >= min_weight.  s(n): the eight tsdf corners interpolated along
 *             x, then y, then z, each as a + f (b - a).
 *   march     n* = the smallest n with s(n) valid and s(n) < 0.  A hit: n* >= 2, s(n* - 1) valid and s(n* - 1) >= 0; then
 *             z* = z_{n* - 1} + step (s0 / (s0 - s1)), disp = fb / z*, fb = fx baseline formed in fp32 on the host.  Every other ray - no
 *             n*, a start inside or behind a surface, a surface reached out of unobserved space - is a miss: 0 in all three outputs.
 *   normal    the gradient of the trilinear interpolant at sample n* in its cell, corners c_xyz: dx_yz = c_1yz - c_0yz,
 *             c_yz = c_0yz + f_x dx_yz, dy_z = c_1z - c_0z, c_z = c_0z + f_y dy_z;
 *             g0 = gx_0 + f_z (gx_1 - gx_0) with gx_z = dx_0z + f_y (dx_1z - dx_0z), g1 = dy_0 + f_z (dy_1 - dy_0), g2 = c_1 - c_0; divided
 *             by sqrt((g0 g0 + g1 g1) + g2 g2): world axes, towards positive tsdf (free space) as the mesh normals; zeros when that length
 *             is zero or not finite.
 *   value     the trilinear vvalue at sample n*.  (Normal and value are taken at the first sample behind the surface, at most one step
 *             from it.)
 * tsdf, weight, vvalue (nz, ny, nx) as dis_tsdf_integrate writes them, R (nv, 3, 3), t (nv, 3): DEVICE.  origin3_host, K4_host: HOST.
 * Outputs, DEVICE, every element written: disp (nv, h, w), normal (nv, 3, h, w), value (nv, h, w), fp32.
 * variant 1, the plain form: one launch; every sample of a ray's range of n - a slab test against the lattice box, widened on both
 * sides; a sample outside the lattice is invalid, so the widening changes no result - reads its eight weights and eight corners.
 * variant 0, the shipped form, gives the same bits from three launches: the state of every cell (0: a corner weight below min_weight,
 * 1: all observed and none negative, 2: all observed and one negative; a + f (b - a) cannot be negative between non-negative corners, so
 * only state-2 cells are gathered), the number of state-2 cells of every brick of 8 x 8 x 8 cells (a ray inside a brick without one
 * jumps to its last sample that still lies inside that brick), the march.  A wave takes an 8 x 8 tile of pixels.
 * No atomics, no allocation, no synchronisation: two calls give the same bits, and the call is capturable.
 * workspace: dis_tsdf_raycast_workspace(nx, ny, nz) BYTES (-1: unsupported extents), 16-byte aligned, no initialisation; after a call
 * of variant 0 it holds the cell states (nz - 1, ny - 1, nx - 1) uint8 at byte 0 and, at the next multiple of 16, the state-2 counts of
 * the bricks (ceil((nz - 1) / 8), ceil((ny - 1) / 8), ceil((nx - 1) / 8)) int32.
 * Checks, in this order, all before any launch: a NULL pointer -> DIS_ERR_NULL; nv outside 1 .. 64, h or w outside 2 .. 8192, nx, ny or nz
 * outside 2 .. 1024 -> DIS_ERR_BAD_SHAPE; fx, fy, baseline, fx baseline or voxel not positive and finite, cx, cy or a component of the
 * origin not finite, min_weight outside 1 .. 4, step outside voxel / 8 .. 8 voxel, (the lattice's diagonal in voxels) voxel / step - a
 * bound on the samples a ray has inside the lattice - not below 2^24 (float(n) must stay exact), workspace_bytes below
 * dis_tsdf_raycast_workspace(...), a misaligned workspace, a variant other than 0 or 1 -> DIS_ERR_UNSUPPORTED. */
long dis_tsdf_raycast_workspace(int nx, int ny, int nz);
int dis_tsdf_raycast(const float* tsdf, const unsigned char* weight, const float* vvalue, const float* origin3_host, float voxel,
                     int min_weight, const float* R, const float* t, const float* K4_host, float baseline, float step, int variant,
                     float* disp, float* normal, float* value, int nv, int h, int w, int nx, int ny, int nz, void* workspace,
                     long workspace_bytes, void* stream);

/* dis_tsdf_align_poses: frame-to-model pose refinement (csrc/tsdf_align.hip): the poses of nv views - a track's frames, say - refined
 * against a volume, by Gauss-Newton on the signed distance of every view's back-projected pixels to the volume's surface.  No flow and
 * no second frame are read.  tests/tsdf_align_ref.py restates it in numpy, operand order included.  Every per-pixel term is a fixed
 * fp32 expression, converted to fp64 and added in fp64; the state and the solve are fp64, as in "track poses", and the layout of the 30
 * sums, the reduction and the 6 x 6 step are those of dis_track_poses.  fb = fx baseline, s2 = scale scale and tv = trunc / voxel are
 * formed in fp32 on the host.  Per view, per pass at the state (R, t) rounded to fp32, the pixel (u, v) with disparity d:
 *   skipped unless d is valid.  P = (z ((float(u) - cx) / fx), z ((float(v) - cy) / fy), z), z = fb / d.
 *   q = P - t; X_k = (R[0][k] q0 + R[1][k] q1) + R[2][k] q2 (the world point); g_a = (X_a - origin_a) / voxel.
 *   The cell and its inside test are those of dis_tsdf_raycast: skipped unless 0 <= g_a < float(n_a - 1) on the three axes; i_a =
 *   floor(g_a), f_a = g_a - float(i_a); skipped unless the eight corner weights are >= min_weight.
 *   s = the trilinear tsdf (x, then y, then z, each a + f (b - a)); skipped unless |s| < 1: saturated free space has no gradient.
 *   (g0, g1, g2) = the gradient of the interpolant in lattice units, the expressions of dis_tsdf_raycast's normal before its division.
 *   e = trunc s, the residual: a length.  m_a = tv g_a; n_r = (R[r][0] m0 + R[r][1] m1) + R[r][2] m2, the gradient of e in the camera's
 *   frame.  J = (n1 P2 - n2 P1, n2 P0 - n0 P2, n0 P1 - n1 P0, -n0, -n1, -n2): rotation 0 .. 2, translation 3 .. 5 of the left
 *   perturbation R <- dR R, t <- dR t + delta.  wgt = g g with g = 1 / (1 + (e e) / s2), in every pass: the start is assumed near.
 *   H_pq += (wgt J_p) J_q for p <= q, g_p += (wgt J_p) e, S_w += wgt, S_c += wgt (e e), n += 1.
 * The step: as in dis_track_poses - fewer than min_corr used pixels, or a pivot of the Cholesky factorisation of H + damping diag(H)
 * that is not > 0 and finite, fails the view, which keeps its last good state: R_init, t_init bit for bit if the first pass fails.
 * tsdf, weight (nz, ny, nx) as dis_tsdf_integrate writes them, disp (nv, h, w), R_init (nv, 3, 3), t_init (nv, 3) (X_c = R X_w + t):
 * DEVICE.  origin3_host, K4_host: HOST.  Outputs, DEVICE, every element written: R (nv, 3, 3), t (nv, 3), stats (nv, 8) fp32 =
 * {n, S_w / n, sqrt(S_c / S_w), status (1 ok, 0 failed)} of the closing pass, {n, S_w / n, sqrt(S_c / S_w)} of the opening pass at
 * R_init, the number of valid disparities of the view (a ratio without a denominator is 0).
 * iters + 1 launches of tsdf_align_accum_kernel (bpp workgroups of 256 lanes per view, a wave per 8 x 8 patch of a 16 x 16 tile, the
 * tiles of a view taken in turn by its workgroups; one record of 32 doubles per workgroup) and iters + 1 of tsdf_align_solve_kernel (a
 * wave per view; the records added in ascending order), in turn on the given stream; the last pair only measures.  The hand-off is
 * the launch boundary alone: no atomics, no flags polled between workgroups, no allocation, no synchronisation - two calls give the
 * same bits, a view's result does not depend on the other views of the call, and the call is capturable.  The first accumulate launch
 * reads R_init directly: the workspace needs no initialisation.
 * workspace: dis_tsdf_align_workspace(nv, h, w) BYTES (-1: unsupported extents), 16-byte aligned.
 * Checks, in this order, all before any launch: a NULL pointer -> DIS_ERR_NULL; nv outside 1 .. 64, h or w outside 2 .. 8192, nx, ny or
 * nz outside 2 .. 1024 -> DIS_ERR_BAD_SHAPE; iters outside 1 .. 64, scale, scale scale, voxel, trunc, trunc / voxel, fx, fy, baseline or
 * fx baseline not positive and finite, damping negative or not finite, min_corr < 6, min_weight outside 1 .. 4, cx, cy or a component of
 * the origin not finite, workspace_bytes below dis_tsdf_align_workspace(...), a misaligned workspace -> DIS_ERR_UNSUPPORTED. */
long dis_tsdf_align_workspace(int nv, int h, int w);
int dis_tsdf_align_poses(const float* tsdf, const unsigned char* weight, const float* origin3_host, float voxel, float trunc,
                         int min_weight, const float* disp, const float* K4_host, float baseline, const float* R_init,
                         const float* t_init, int iters, float scale, float damping, int min_corr, float* R, float* t, float* stats,
                         int nv, int h, int w, int nx, int ny, int nz, void* workspace, long workspace_bytes, void* stream);

/* ---------------------------------------------------------------- optimiser ----------------- */

/* torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8) on a flat fp32 buffer (reference train_val.py:55-56).
 * step_count is the 1-based step index; grads are multiplied by grad_scale first (1/world_size for DP).  The betas are
 * doubles: torch.optim.Adam evaluates (1 - beta) and beta^t on python floats and rounds once. */
int dis_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long count, float lr,
                  double beta1, double beta2, float eps, int step_count, float grad_scale, void* stream);
/* The same update with the step counter on the device: state = 4 x 32 bit {int steps taken, float 1-beta1^t,
 * float sqrt(1-beta2^t), unused}, advanced by the call itself.  Safe to capture in a hipGraph: replay k applies
 * step k's bias correction (dis_adam_step would replay the capture-time correction). */
int dis_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long count, float lr,
                      double beta1, double beta2, float eps, int* state, float grad_scale, void* stream);
/* dis_adam_step_dev with the hyper-parameters and the clip / skip decision on the device as well, so that a captured step
 * honours a learning rate changed between replays and clips without the host looking at the gradient.
 *   hyper:    4 floats on the DEVICE {learning rate, max_norm (read only when mode & 1), reserved, reserved}.
 *   state:    as in dis_adam_step_dev.
 *   mode:     bit 0: clip by global L2 norm, coefficient min(1, max_norm / (norm + 1e-6)) in fp64 (torch.nn.utils.clip_grad_norm_;
 *             a non-finite norm without bit 1 gives a NaN coefficient that propagates, as in torch); bit 1: skip the step - param,
 *             moments and state untouched - when the squared norm is not finite (gradients of 1e30 are finite: sums are fp64).
 *             0: no norm pass, two launches, the bits of dis_adam_step_dev at the same learning rate; so is any step whose
 *             coefficient is exactly 1.
 *   stats:    4 doubles on the DEVICE, written when mode != 0: {L2 norm of grad * grad_scale, coefficient applied, running count of
 *             skipped steps (only ever incremented: zero it once), 1.0 if this call skipped else 0.0}.
 *   partials: dis_adam_step_hyper_workspace(count) doubles (< 0: unsupported count); needs no initialisation.  stats and partials
 *             may be NULL when mode == 0.
 * The norm repeats bit for bit, on any device: one workgroup per fixed-size range of `grad`, every summation order fixed, no atomics.
 * No host synchronisation, no allocation: safe to capture.  `mode` decides which kernels are launched - a property of the capture. */
long dis_adam_step_hyper_workspace(long count);
int dis_adam_step_hyper(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long count, const float* hyper,
                        double beta1, double beta2, float eps, int* state, double* stats, double* partials, int mode,
                        float grad_scale, void* stream);

/* ---------------------------------------------------------------- gradient exchange -------- */

/* The data-parallel step's collective behind the C ABI (ONE all-reduce of the flat fp32 gradient per
 * step, mean of the per-rank gradients; the reference itself is single-GPU, train_val.py:55-56, and has no counterpart).  RCCL is
 * bound at the first call (dlopen by soname: a process that already holds torch's copy keeps ONE RCCL); DIS_ERR_UNSUPPORTED when no
 * librccl can be found.  RCCL's own errors come back as 10000 + ncclResult_t.
 *   dis_allreduce_unique_id: rank 0 fills 128 bytes (ncclUniqueId) and hands them to the other ranks by its own means;
 *   dis_allreduce_init:      every rank, collectively; *comm is an opaque handle owned by the caller (dis_allreduce_destroy);
 *   dis_allreduce_sum_f32:   in place on `count` floats of device memory, asynchronous on `stream`; average != 0: the sum / nranks
 *                            (ncclAvg) - the DP mean, so that dis_adam_step runs with grad_scale 1; count 0 is a no-op.
 * One process per GPU, the device current at dis_allreduce_init is the communicator's. */
int dis_allreduce_unique_id(void* id128);
int dis_allreduce_init(void** comm, const void* id128, int nranks, int rank);
int dis_allreduce_sum_f32(void* comm, float* buf, long count, int average, void* stream);
int dis_allreduce_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif
