// Batch assembly for packed track files (depthinspace_amd/data/packed.py): bs raw records + the per-sample frame order ->
// the step's inputs in their final (tl, bs, ...) layout, in ONE launch.  A plain streaming copy: no LDS, no atomics, every
// output element written exactly once (replay-safe in front of a captured step).
#include "common.h"

#define TRK_PLANE_FIELDS 6   // im, ambient, disp, sgm_disp, primary_disp, pseudo_gt: (4, h, w) per record, one plane per frame
#define TRK_BLOCK 256
#define TRK_UNROLL 4         // vectors per thread and tile: independent loads in flight before the first store

struct TrkArgs {
  const float* raw;
  const int* perm;
  long stride;                        // floats between two records
  long src[TRK_PLANE_FIELDS];         // float offset of the field inside a record (present fields only, packed to the front)
  float* dst[TRK_PLANE_FIELDS];
  int nf;                             // number of present plane fields
  long src_flow, src_R, src_t;        // src_flow < 0: no flow output
  float *dst_flow, *dst_R, *dst_t;
  int bs, tl;
  long hw;
};

// pair(p, q) = 3p + q - (q > p): position of flow_pq in the file order 01 02 03 10 12 13 20 21 23 30 31 32
__device__ __forceinline__ int trk_pair(int p, int q) { return 3 * p + q - (q > p ? 1 : 0); }

// One tile = TRK_BLOCK * TRK_UNROLL vectors of one (h, w) plane; the plane (field, frame slot, sample - or flow pair, sample, channel)
// is block-uniform, so the index arithmetic is scalar.  The last tile copies R and t.  T: float4 (16 bytes per lane) or float.
template <typename T>
__global__ void __launch_bounds__(TRK_BLOCK) assemble_tracks_kernel(const TrkArgs a, const long n_per_plane, const long tiles_per_plane,
                                                                    const long n_tiles) {
  const long plane_planes = (long)a.nf * a.tl * a.bs;
  for (long tile = blockIdx.x; tile <= n_tiles; tile += gridDim.x) {
    if (tile == n_tiles) {   // R (tl, bs, 3, 3) and t (tl, bs, 3): 12 floats per (frame slot, sample)
      const int n = a.tl * a.bs;
      for (int e = threadIdx.x; e < n * 12; e += TRK_BLOCK) {
        const int r = e / 12, c = e % 12, i = r / a.bs, b = r % a.bs;
        const int f = a.perm[b * a.tl + i] & 3;   // masked: no table content can address outside a record
        const float* rec = a.raw + (long)b * a.stride;
        if (c < 9) a.dst_R[r * 9 + c] = rec[a.src_R + f * 9 + c];
        else a.dst_t[r * 3 + (c - 9)] = rec[a.src_t + f * 3 + (c - 9)];
      }
      continue;
    }
    const long q = tile / tiles_per_plane;
    const long e0 = (tile % tiles_per_plane) * (TRK_BLOCK * TRK_UNROLL) + threadIdx.x;
    const float* s = nullptr;   // nullptr: a zero plane
    float* d;
    if (q < plane_planes) {
      const int f = (int)(q / ((long)a.tl * a.bs)), r = (int)(q % ((long)a.tl * a.bs));
      const int i = r / a.bs, b = r % a.bs;
      const int fr = a.perm[b * a.tl + i] & 3;
      s = a.raw + (long)b * a.stride + a.src[f] + (long)fr * a.hw;
      d = a.dst[f] + (long)r * a.hw;
    } else {   // flows: (tl * tl, bs, 2, h, w), plane = ((i * tl + j) * bs + b) * 2 + channel
      const long qf = q - plane_planes;
      const int c = (int)(qf & 1), r = (int)(qf >> 1);
      const int b = r % a.bs, ij = r / a.bs, i = ij / a.tl, j = ij % a.tl;
      const int p0 = a.perm[b * a.tl + i] & 3, p1 = a.perm[b * a.tl + j] & 3;
      if (i != j && p0 != p1)   // (p0 == p1 for i != j is not a frame order; such a plane is written as zeros, never read out of range)
        s = a.raw + (long)b * a.stride + a.src_flow + (long)(trk_pair(p0, p1) * 2 + c) * a.hw;
      d = a.dst_flow + qf * a.hw;
    }
    const T* sv = (const T*)s;
    T* dv = (T*)d;
    T v[TRK_UNROLL];
#pragma unroll
    for (int k = 0; k < TRK_UNROLL; ++k) {
      const long e = e0 + (long)k * TRK_BLOCK;
      v[k] = T{};
      if (s && e < n_per_plane) v[k] = sv[e];
    }
#pragma unroll
    for (int k = 0; k < TRK_UNROLL; ++k) {
      const long e = e0 + (long)k * TRK_BLOCK;
      if (e < n_per_plane) dv[e] = v[k];
    }
  }
}

static inline bool trk_inside(long off, long size, long stride) { return off >= 0 && off <= stride && size <= stride - off; }
static inline bool trk_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int dis_assemble_tracks(const float* raw, long record_stride, const int* perm, const DisTrackLayout* layout,
                                   const DisTrackOut* out, int bs, int tl, int h, int w, void* stream) {
  if (!raw || !perm || !layout || !out) return DIS_ERR_NULL;
  if (!out->im || !out->ambient || !out->disp || !out->R || !out->t) return DIS_ERR_NULL;
  if (bs <= 0 || tl <= 0 || h <= 0 || w <= 0 || tl > 4) return DIS_ERR_BAD_SHAPE;
  const long hw = (long)h * w;
  if (hw > (1L << 40) || (long)bs * tl > (1L << 24)) return DIS_ERR_BAD_SHAPE;   // (the index arithmetic below stays far inside 64 bits)
  // field table: offset in the record, size in floats, destination
  const long offs[9] = {layout->im, layout->ambient, layout->disp, layout->sgm_disp, layout->primary_disp, layout->pseudo_gt,
                        layout->flow, layout->R, layout->t};
  float* const dsts[9] = {out->im, out->ambient, out->disp, out->sgm_disp, out->primary_disp, out->pseudo_gt,
                          out->flow, out->R, out->t};
  const long sizes[9] = {4 * hw, 4 * hw, 4 * hw, 4 * hw, 4 * hw, 4 * hw, 24 * hw, 36, 12};
  for (int k = 0; k < 9; ++k)   // -1: absent; anything else has to lie inside the record
    if (offs[k] != -1 && !trk_inside(offs[k], sizes[k], record_stride)) return DIS_ERR_BAD_SHAPE;
  for (int k = 0; k < 9; ++k)
    if (dsts[k] && offs[k] == -1) return DIS_ERR_UNSUPPORTED;
  TrkArgs a;
  a.raw = raw; a.perm = perm; a.stride = record_stride; a.bs = bs; a.tl = tl; a.hw = hw;
  a.nf = 0;
  bool vec = hw % 4 == 0 && record_stride % 4 == 0 && trk_al16(raw);
  for (int k = 0; k < TRK_PLANE_FIELDS; ++k) {
    a.src[k] = 0; a.dst[k] = nullptr;
    if (!dsts[k]) continue;
    a.src[a.nf] = offs[k]; a.dst[a.nf] = dsts[k]; ++a.nf;
    vec = vec && offs[k] % 4 == 0 && trk_al16(dsts[k]);
  }
  a.src_flow = out->flow ? layout->flow : -1; a.dst_flow = out->flow;
  if (out->flow) vec = vec && layout->flow % 4 == 0 && trk_al16(out->flow);
  a.src_R = layout->R; a.dst_R = out->R; a.src_t = layout->t; a.dst_t = out->t;
  const long planes = (long)a.nf * tl * bs + (out->flow ? 2L * tl * tl * bs : 0);
  const long n_per_plane = vec ? hw / 4 : hw;
  const long tiles_per_plane = (n_per_plane + TRK_BLOCK * TRK_UNROLL - 1) / (TRK_BLOCK * TRK_UNROLL);
  const long n_tiles = planes * tiles_per_plane;
  const dim3 grid(dis_ew_grid((n_tiles + 1) * TRK_BLOCK, TRK_BLOCK)), block(TRK_BLOCK);
  if (vec)
    hipLaunchKernelGGL(assemble_tracks_kernel<float4>, grid, block, 0, (hipStream_t)stream, a, n_per_plane, tiles_per_plane, n_tiles);
  else
    hipLaunchKernelGGL(assemble_tracks_kernel<float>, grid, block, 0, (hipStream_t)stream, a, n_per_plane, tiles_per_plane, n_tiles);
  DIS_CHECK_LAUNCH();
  return DIS_OK;
}
