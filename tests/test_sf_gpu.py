"""DIS-SF on the HIP path: the streaming MFMA convolution family (csrc/conv_gen.hip) through the C ABI vs plain
PyTorch fp32 CPU references, the DispNetS forward/backward vs the CPU oracle (incl. the crop_like path), and the
whole DIS-SF / DIS-FTSF training step vs the reference goldens (tests/golden/sf_*.npz, produced by
oracle/make_golden.py from the imported reference).
The bars of the per-layer tables here (2e-5 / 5e-5 of the largest entry) are what real-valued data allows; a single lost, doubled or
misplaced term - in particular one second-plane term of the two-term split - stays below them: tests/test_convg_exact_gpu.py holds
the same kernels to float64 bit for bit on wide-integer operands and pins the kernel every call reaches."""
import os
import argparse
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import dis_oracle as O


def relerr(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# cin (weight), cin_mem (padded buffer), cout, k, stride, h, w: the DispNetS layer shapes at small spatial sizes
CONVG_SHAPES = [
    (2, 4, 32, 7, 2, 40, 36),      # conv1.0 (2-channel input in a 4-channel buffer)
    (32, 32, 32, 7, 1, 20, 18),    # conv1.2
    (32, 32, 64, 5, 2, 21, 19),    # conv2.0, odd sizes
    (64, 64, 64, 5, 1, 11, 10),    # conv2.2
    (64, 64, 128, 3, 2, 14, 7),    # conv3.0
    (256, 256, 512, 3, 2, 8, 7),   # conv5.0
    (512, 512, 512, 3, 1, 4, 4),   # conv7.2
    (1024, 1024, 512, 3, 1, 8, 7),  # iconv7
    (129, 132, 64, 3, 1, 16, 14),  # iconv3: concat with one disparity channel, zero-padded to 132
    (17, 20, 16, 3, 1, 32, 27),    # iconv1
]


@pytest.mark.parametrize('cin,cin_mem,cout,k,stride,h,w', CONVG_SHAPES)
def test_convg_conv_fwd_bwd(cin, cin_mem, cout, k, stride, h, w):
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout + k)
    n, pad = 2, (k - 1) // 2
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.relu(F.conv2d(xr, wr, br, stride=stride, padding=pad))
    go = torch.randn(y.shape, generator=g)
    y.backward(go)

    xp = torch.zeros(n, h, w, cin_mem)
    xp[..., :cin] = nhwc(x)
    xd = xp.cuda().requires_grad_(True)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    yd = ops.convg(xd, wd, bd, stride, pad, ops.ACT_RELU)
    assert tuple(yd.shape) == (n, y.shape[2], y.shape[3], cout)
    assert relerr(nchw(yd), y) < 2e-5
    yd.backward(nhwc(go).cuda())
    assert relerr(nchw(xd.grad[..., :cin]), xr.grad) < 5e-5
    if cin_mem > cin:
        assert float(xd.grad[..., cin:].abs().max()) == 0.0
    assert relerr(wd.grad, wr.grad) < 5e-5
    assert relerr(bd.grad, br.grad) < 5e-5


@pytest.mark.parametrize('case', ['randn', 'outlier_pixel', 'tiny_image', 'dominant_weight', 'heavy_tailed_grad'])
@pytest.mark.parametrize('cin,cout,k,stride,h,w', [(64, 64, 5, 1, 22, 20), (256, 512, 3, 2, 16, 14), (128, 64, 3, 1, 24, 27)])
def test_convg_f16x2_streaming_is_fp32_accurate(case, cin, cout, k, stride, h, w):
    """The streaming convolutions of DispNetS with >= 32 input channels on the two-term fp16 split (convg2_fwd_kernel: 3 products,
    one power-of-two scale per IMAGE of x and one for the weights) against fp64, beside the three-term bf16 kernel (6 products, no
    scaling) on the same inputs; forward and input gradient (the same kernel in its transposed mode).  Bar: 4 x the bf16x3
    kernel's error + 2e-7, of the largest entry - overall, and PER IMAGE (each image has its own scale):
      outlier_pixel   one pixel of 1e4 in image 0: that image's scale is set by the outlier (its other outputs keep an absolute
                      error of 2^-39 of it), image 1 is untouched;
      tiny_image      image 1 is 1e-6 x image 0: its own scale, full relative accuracy;
      dominant_weight one weight 1e3 x the rest;
      heavy_tailed_grad (round-4 advice) the OUTPUT gradient - the operand of the transposed mode - spans 1e6 WITHIN each image
                      (its right half is 1e-6 x its left half): the one scale per image keeps the absolute error at 2^-39 of the
                      image's largest entry (the bar below), and the small half's input gradient, judged on its own, still holds
                      ~1e-3 relative accuracy (14 of its bits survive the fp16 planes 2^20 below the scale) - what a gradient that
                      is a millionth of its neighbours' contributes to a sum."""
    from depthinspace_amd import ops
    from tests.conftest import conv_split
    g = torch.Generator().manual_seed(cin + cout + k + len(case))
    n, pad = 2, (k - 1) // 2
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    if case == 'outlier_pixel':
        x[0, :, h // 2, w // 3] = 1e4
    elif case == 'tiny_image':
        x[1] *= 1e-6
    elif case == 'dominant_weight':
        wt[3, 5, k // 2, k // 2] *= 1e3
    b = torch.randn(cout, generator=g) * (0.1 if case != 'tiny_image' else 0.0)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(xr, wr, b.double(), stride=stride, padding=pad)
    go = torch.randn(y.shape, generator=g)
    if case == 'tiny_image':
        go[1] *= 1e-6
    if case == 'heavy_tailed_grad':
        go[..., go.shape[-1] // 2:] *= 1e-6
    y.backward(go.double())
    out = {}
    for tag in ('bf16x3', 'f16x2'):
        with conv_split(tag):
            xd = nhwc(x).cuda().requires_grad_(True)
            wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
            yd = ops.convg(xd, wd, bd, stride, pad, ops.ACT_NONE)
            yd.backward(nhwc(go).cuda())
            out[tag] = (nchw(yd).detach().double().cpu(), nchw(xd.grad).double().cpu())

    def err(a, ref):
        return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))
    for name, i, ref in (('y', 0, y.detach()), ('gx', 1, xr.grad)):
        e3, e2 = err(out['bf16x3'][i], ref), err(out['f16x2'][i], ref)
        per3 = [err(out['bf16x3'][i][q], ref[q]) for q in range(n)]
        per2 = [err(out['f16x2'][i][q], ref[q]) for q in range(n)]
        print(f'{case} {cin}->{cout} k{k} s{stride} {name}: bf16x3 {e3:.2e} {per3}  f16x2 {e2:.2e} {per2}')
        assert e2 < 4 * e3 + 2e-7, (case, name, e3, e2)
        for q in range(n):
            assert per2[q] < 4 * per3[q] + 2e-7, (case, name, q, per3[q], per2[q])
    if case == 'heavy_tailed_grad' and stride == 1:
        # the region whose incoming gradients are a millionth of the image's largest (two window widths away from the border
        # between the halves), relative to ITS OWN largest entry
        c0 = w // 2 + k
        small, sref = out['f16x2'][1][..., c0:], xr.grad[..., c0:]
        e_small = float((small - sref).abs().max() / sref.abs().max())
        print(f'  small half of gx, relative to its own largest entry: {e_small:.2e}')
        assert e_small < 5e-3, e_small


class halo_min(object):
    """context manager: DIS_CONVG_HALO_MIN for a block (the smallest output grid, in pixels, whose fp32 streaming convolutions
    take the LDS-halo form convh2_kernel; the library reads it per call)"""

    def __init__(self, v):
        self.v = str(v)

    def __enter__(self):
        self.prev = os.environ.get('DIS_CONVG_HALO_MIN')
        os.environ['DIS_CONVG_HALO_MIN'] = self.v

    def __exit__(self, *a):
        if self.prev is None:
            os.environ.pop('DIS_CONVG_HALO_MIN', None)
        else:
            os.environ['DIS_CONVG_HALO_MIN'] = self.prev
        return False


def _kernels_of(fn_):
    """run fn_ under lib's per-call recorder -> (result, set of kernel tags the dis_convg_run calls reported)"""
    from depthinspace_amd import lib
    lib.profile_start()
    out = fn_()
    rec = lib.profile_stop()
    return out, {t for (name, _, _, t, _) in rec if name == 'dis_convg_run'}


# kind, cin, cin_mem, cout, k, stride, h, w (conv: input size; tconv: input size, output = 2h-? x 2w-? given below)
HALO_SHAPES = [
    ('conv', 32, 32, 32, 7, 1, 37, 41),     # conv1.2: 49 taps, streaming weight groups, 16-row tiles, ragged edges
    ('conv', 32, 32, 64, 5, 2, 45, 38),     # conv2.0: stride 2 (large halo)
    ('conv', 64, 64, 64, 5, 1, 33, 35),     # conv2.2: two 32-channel chunks
    ('conv', 64, 64, 128, 3, 2, 40, 36),    # conv3.0: two cout blocks
    ('conv', 129, 132, 64, 3, 2, 34, 33),   # a padded concat buffer (zero weights beyond channel 129), 5 chunks
    ('conv', 64, 64, 4, 5, 1, 36, 40),      # a partial cout block (4 of 16)
    ('tconv', 32, 32, 16, 3, 2, 33, 38),    # upconv1: 4 parity classes of 1 - 4 taps, resident weights
    ('tconv', 64, 64, 32, 3, 2, 32, 35),    # upconv2 with a crop
    ('tconv', 128, 128, 64, 3, 2, 35, 32),
]


@pytest.mark.parametrize('kind,cin,cin_mem,cout,k,stride,h,w', HALO_SHAPES)
def test_convg_f16x2_halo_form(kind, cin, cin_mem, cout, k, stride, h, w):
    """convh2_kernel (two-term fp16, input halo staged in LDS once per tile and 32-channel chunk) against fp64 and beside the
    streaming kernel convg2_fwd_kernel on the same inputs: forward and input gradient (which runs the same kernel in its other
    mode: stride-2 input gradients and transposed convolutions as four parity classes).  Both forms split the operands into the
    same two fp16 terms under power-of-two block scales (the streaming kernel one per image, the halo form a running one per tile;
    one for the weights), so their errors against fp64 are of one size: bar 3 x streaming + 2e-7.  Image 1 is 37 x the others:
    a halo stage never mixes images, a chunk with a larger magnitude than its predecessors rescales the accumulators."""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin + cout + k + h)
    n, pad = 3, (k - 1) // 2
    x = torch.randn(n, cin, h, w, generator=g)
    x[1] *= 37.0    # (images with different scales)
    if cin > 32:
        x[:, 32:64] *= 50.0   # (... and a second 32-channel chunk far above the first: the running scale must shrink there)
    b = torch.randn(cout, generator=g) * 0.1
    if kind == 'conv':
        wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        xr = x.double().requires_grad_(True)
        y = F.conv2d(xr, wt.double(), b.double(), stride=stride, padding=pad)
    else:
        wt = torch.randn(cin, cout, 3, 3, generator=g) / (cin * 9) ** 0.5
        xr = x.double().requires_grad_(True)
        hout, wout = 2 * h - (h % 2), 2 * w - 1   # crop_like targets: one with, one without a cropped row
        y = F.conv_transpose2d(xr, wt.double(), b.double(), stride=2, padding=1, output_padding=1)[:, :, :hout, :wout]
    go = torch.randn(y.shape, generator=g)
    y.backward(go.double())
    xp = torch.zeros(n, h, w, cin_mem)
    xp[..., :cin] = nhwc(x)

    def run():
        xd = xp.cuda().requires_grad_(True)
        wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        if kind == 'conv':
            yd = ops.convg(xd, wd, bd, stride, pad, ops.ACT_NONE)
        else:
            yd = ops.convg_transposed(xd, wd, bd, (y.shape[2], y.shape[3]), 1, ops.ACT_NONE)
        yd.backward(nhwc(go).cuda())
        return nchw(yd).detach().double().cpu(), nchw(xd.grad[..., :cin]).double().cpu(), wd.grad.double().cpu()
    with halo_min(1):
        halo, tags_h = _kernels_of(run)
    with halo_min(1 << 40):
        stream, tags_s = _kernels_of(run)
    assert any('convh2_kernel' in t for t in tags_h), tags_h
    assert not any('convh2_kernel' in t for t in tags_s), tags_s

    def err(a, ref):
        return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))
    for name, i, ref in (('y', 0, y.detach()), ('gx', 1, xr.grad)):
        eh, es = err(halo[i], ref), err(stream[i], ref)
        print(f'{kind} {cin}->{cout} k{k} s{stride} {name}: halo {eh:.2e} streaming {es:.2e}  kernels {sorted(tags_h)}')
        assert eh < 3 * es + 2e-7, (name, eh, es)
        for q in range(n):
            assert err(halo[i][q], ref[q]) < 3 * err(stream[i][q], ref[q]) + 2e-7, (name, q)
    assert err(halo[2], stream[2]) < 1e-6   # (the weight gradient does not depend on the form)


@pytest.mark.parametrize('cin,cout,stride,h,w', [(128, 512, 1, 80, 84), (256, 128, 1, 160, 164), (256, 256, 2, 180, 176)])
def test_convg_f16x2_large_tiles(cin, cout, stride, h, w):
    """convg2_fwd_kernel<128, 8> (eight waves on a 256-pixel x 128-cout tile: the deep layers of DispNetS at bench scale, where the
    launch still fills the device) against fp64, beside the three-term kernel on its 128 x 64 tiles: forward and input gradient.
    The maps here are large enough for the large tile and are kept out of the halo form (DIS_CONVG_HALO_MIN)."""
    from depthinspace_amd import ops
    from tests.conftest import conv_split
    g = torch.Generator().manual_seed(cin + cout + h)
    n, k, pad = 2, 3, 1
    x = torch.randn(n, cin, h, w, generator=g)
    x[1] *= 0.01
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xr = x.double().requires_grad_(True)
    y = F.conv2d(xr, wt.double(), b.double(), stride=stride, padding=pad)
    go = torch.randn(y.shape, generator=g)
    y.backward(go.double())
    out, tags = {}, {}
    for tag in ('bf16x3', 'f16x2'):
        with conv_split(tag), halo_min(1 << 40):
            def run():
                xd = nhwc(x).cuda().requires_grad_(True)
                wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
                yd = ops.convg(xd, wd, bd, stride, pad, ops.ACT_NONE)
                yd.backward(nhwc(go).cuda())
                return nchw(yd).detach().double().cpu(), nchw(xd.grad).double().cpu()
            out[tag], tags[tag] = _kernels_of(run)
    assert any('256 x 128 tiles' in t for t in tags['f16x2']), tags['f16x2']

    def err(a, ref):
        return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))
    for name, i, ref in (('y', 0, y.detach()), ('gx', 1, xr.grad)):
        e3, e2 = err(out['bf16x3'][i], ref), err(out['f16x2'][i], ref)
        print(f'{cin}->{cout} s{stride} {name}: bf16x3 {e3:.2e} f16x2 (large tiles) {e2:.2e}  kernels {sorted(tags["f16x2"])}')
        assert e2 < 4 * e3 + 2e-7, (name, e3, e2)
        for q in range(n):
            assert err(out['f16x2'][i][q], ref[q]) < 4 * err(out['bf16x3'][i][q], ref[q]) + 2e-7, (name, q)


# cin, cout, hin, win, hout, wout (crop_like target)
TCONV_SHAPES = [
    (512, 512, 4, 4, 8, 7),     # upconv7 at 512x432: 8x8 cropped to 8x7
    (512, 256, 16, 14, 32, 27),  # upconv5: 32x28 cropped to 32x27
    (64, 32, 12, 9, 24, 18),    # upconv2, no crop
    (32, 16, 10, 11, 19, 21),   # upconv1 with a crop in both directions
]


@pytest.mark.parametrize('cin,cout,hin,win,hout,wout', TCONV_SHAPES)
def test_convg_transposed_fwd_bwd(cin, cout, hin, win, hout, wout):
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin + cout + hin)
    n = 2
    x = torch.randn(n, cin, hin, win, generator=g)
    wt = torch.randn(cin, cout, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.relu(F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1))[:, :, :hout, :wout]
    go = torch.randn(y.shape, generator=g)
    y.backward(go)

    xd = nhwc(x).cuda().requires_grad_(True)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    yd = ops.convg_transposed(xd, wd, bd, (hout, wout), 1, ops.ACT_RELU)
    assert relerr(nchw(yd), y) < 2e-5
    yd.backward(nhwc(go).cuda())
    assert relerr(nchw(xd.grad), xr.grad) < 5e-5
    assert relerr(wd.grad, wr.grad) < 5e-5
    assert relerr(bd.grad, br.grad) < 5e-5


@pytest.mark.parametrize('cin,alpha', [(128, 16.0), (64, 32.0), (32, 64.0), (16, 128.0)])
def test_convg_head_fwd_bwd(cin, alpha):
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin)
    n, h, w = 2, 13, 17
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(1, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(1, generator=g) * 0.1 + 3.0
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = alpha * torch.sigmoid(F.conv2d(xr, wr, br, padding=1) - 3)
    go = torch.randn(y.shape, generator=g)
    y.backward(go)
    xd = nhwc(x).cuda().requires_grad_(True)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    yd = ops.disp_head_g(xd, wd, bd, alpha, 3.0)
    assert tuple(yd.shape) == (n, 1, h, w)
    assert relerr(yd, y) < 2e-5
    yd.backward(go.cuda())
    assert relerr(nchw(xd.grad), xr.grad) < 5e-5
    assert relerr(wd.grad, wr.grad) < 5e-5
    assert relerr(bd.grad, br.grad) < 5e-5


def test_convg_rejects_bad_arguments():
    from depthinspace_amd import ops, lib
    x = torch.zeros(1, 8, 8, 6, device='cuda')  # 6 channels: not a multiple of 4
    w = torch.zeros(16, 6, 3, 3, device='cuda')
    with pytest.raises(RuntimeError):
        ops.convg(x, w, None, 1, 1)
    with pytest.raises(RuntimeError):
        ops.convg(torch.zeros(1, 8, 8, 8), torch.zeros(16, 8, 3, 3), None, 1, 1)  # CPU tensors: no fallback


@pytest.mark.parametrize('H,W', [(64, 64), (64, 56)])
def test_dispnets_matches_oracle(H, W):
    """DispDecoder forward + parameter gradients vs the CPU oracle; 64x56 exercises crop_like
    (widths 56,28,14,7,4,2,1,1: upconv4 8->7 and upconv7 2->1 are cropped)."""
    from depthinspace_amd.model import networks
    params = O.init_params(O.sf_param_shapes(), seed=5)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 2, H, W, generator=g)
    outs = O.sf_forward(params, x)
    gos = [torch.randn(o.shape, generator=g) for o in outs]
    sum((o * go).sum() for o, go in zip(outs, gos)).backward()

    imsizes = [(H, W)]
    for _ in range(3):
        imsizes.append((imsizes[-1][0] // 2, imsizes[-1][1] // 2))
    net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=imsizes)
    net.load_state_dict({k: v.detach() for k, v in params.items()})
    net = net.cuda()
    outs_d = net(x.cuda())
    assert len(outs_d) == 4
    for o, od in zip(outs, outs_d):
        assert tuple(od.shape) == tuple(o.shape)
        l1 = float((od.detach().cpu() - o.detach()).abs().mean())
        assert l1 < 1e-4, l1
    sum((od * go.cuda()).sum() for od, go in zip(outs_d, gos)).backward()
    worst = 0.0
    for k, p in net.named_parameters():
        e = relerr(p.grad, params[k].grad)
        worst = max(worst, e)
        assert e < 2e-3, (k, e)
    print('DispNetS', H, W, 'worst grad rel err', worst)


def make_args(bs, use_pseudo_gt, data_type='synthetic'):
    return argparse.Namespace(use_pseudo_gt=use_pseudo_gt, lcn_radius=5, track_length=4, data_type=data_type,
                              architecture='single_frame', epochs=1, warmup_epochs=150, train_batch_size=bs,
                              max_disp=128)


@pytest.mark.parametrize('name', ['sf_64_bs1', 'sf_128_bs1_pgt', 'sf_128x108_bs1', 'sf_128_real_pgt', 'sf_64_real_sgm'])
def test_sf_step_matches_reference(golden_dir, name):
    """whole DIS-SF / DIS-FTSF step vs fixtures generated by the imported reference.  sf_128x108_bs1: widths
    108,54,27,14,7,4,2,1 - crop_like (reference model/networks.py:242-263) trims 28->27, 8->7 and 2->1 exactly as at
    512x432.  sf_128_real_pgt: BASELINE config 5 (real pattern, K_processed, baseline 0.0246, pseudo-GT terms).
    sf_64_real_sgm: `real` data in the warm-up epochs: four SGM terms, one per output scale, each with the noise the
    reference drew for it (model/single_frame_worker.py:158-163)."""
    from depthinspace_amd import synth
    from depthinspace_amd.model import networks, single_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    G = np.load(os.path.join(golden_dir, name + '.npz'))
    H, W, bs, pgt = int(G['H']), int(G['W']), int(G['bs']), bool(int(G['use_pseudo_gt']))
    settings = synth.make_settings(H, W, pattern=str(G['pattern']))
    batch = synth.make_batch(settings, bs, 4, seed=int(G['bseed']), with_pseudo_gt=pgt, scene=str(G['scene']),
                             motion=float(G['motion']))
    real_sgm = 'real_sgm' in G.files
    if real_sgm:
        batch['sgm_disp'] = G['sgm_disp']
        for k in range(4):
            batch[f'_sgm_noise{k}'] = G[f'sgm_noise{k}']
    params = O.init_params(O.sf_param_shapes(), seed=int(G['pseed']))
    w = single_frame_worker.Worker(make_args(bs, pgt, 'real' if real_sgm else 'synthetic'), settings=settings)
    w.build_losses()
    w.current_epoch = int(G['epoch'])
    net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes)
    net.load_state_dict({k: v.detach() for k, v in params.items()})
    net = net.cuda()
    opt = FlatAdam(net.parameters(), lr=1e-4)
    errs, outs = w.train_step(net, opt, {k: torch.from_numpy(v) for k, v in batch.items()})
    torch.cuda.synchronize()
    # (ii) the four full-resolution disparities: L1 vs reference < 1e-4 (north-star tolerance)
    assert len(outs) == 4
    for i, o in enumerate(outs):
        ref = torch.from_numpy(G[f'out{i}'])
        l1 = float((o.detach().cpu() - ref).abs().mean())
        assert l1 < 1e-4, (i, l1)
    # (iii) ordered loss terms
    vals = np.array([float(e.detach()) for e in errs])
    assert len(vals) == len(G['vals'])
    np.testing.assert_allclose(vals, G['vals'], rtol=2e-4, atol=2e-6)
    # (iv) gradients of every parameter
    keys = list(G['grad_keys'])
    named = dict(net.named_parameters())
    worst = 0.0
    for i, k in enumerate(keys):
        g = named[k].grad
        scale = float(G['grad_absmax'][i]) + 1e-20
        l2_ref = float(G['grad_l2'][i])
        l2 = float(g.double().norm())
        assert abs(l2 - l2_ref) <= 2e-3 * l2_ref + 1e-12, (k, l2, l2_ref)
        if 'grad:' + k in G.files:
            err = float((g.cpu() - torch.from_numpy(G['grad:' + k])).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-3, (k, err)
    # (v) parameters after one Adam step, where stored: equal to fp32 rounding wherever the reference gradient is well away
    # from 0 (the first Adam step is lr * g / (|g| + eps)); a ~0 gradient may flip its sign: at most 2 lr there
    checked = 0
    for k in keys:
        if 'new:' + k in G.files:
            new_ref = torch.from_numpy(G['new:' + k])
            d = (named[k].detach().cpu() - new_ref).abs()
            if 'grad:' + k in G.files:
                g_ref = torch.from_numpy(G['grad:' + k]).abs()
                sure = g_ref > max(1e-3 * float(g_ref.max()), 1e-6)
                checked += int(sure.sum())
                if bool(sure.any()):
                    assert float(d[sure].max()) <= 1e-6, (k, float(d[sure].max()))
            assert float(d.max()) <= 2.1e-4, k
    assert checked > 1000, checked
    print(name, 'worst grad rel err', worst, 'post-Adam entries checked to 1e-6:', checked)


def test_act_bwd_and_copy_on_channel_ranges():
    """dis_act_bwd_ld / dis_copy_channels: channel ranges of wider nhwc buffers (the in-place decoder concatenations)"""
    from depthinspace_amd import lib, ops
    g = torch.Generator().manual_seed(5)
    npix, c, ldg, ldy = 1000, 24, 40, 32
    gyw = torch.randn(npix, ldg, generator=g).cuda()
    yw = torch.randn(npix, ldy, generator=g).cuda()
    gy, y = gyw[:, 8:8 + c], yw[:, 4:4 + c]
    for act in (ops.ACT_RELU, ops.ACT_SELU, ops.ACT_NONE):
        gp = torch.empty(npix, c, device='cuda')
        lib.call('dis_act_bwd_ld', gy, ldg, y if act != ops.ACT_NONE else None, ldy, gp, act, npix, c)
        ref = torch.empty(npix, c, device='cuda')
        if act == ops.ACT_NONE:
            ref.copy_(gy)
        else:
            lib.call('dis_act_bwd', gy.contiguous(), y.contiguous(), ref, act, npix * c)
        assert torch.equal(gp, ref)
    # one channel + 3 zero lanes (the float4 path) and a general range with a zero tail
    dst = torch.full((npix, 20), 9.0, device='cuda')
    src = torch.randn(npix, 1, generator=g).cuda()
    lib.call('dis_copy_channels', src, 1, dst[:, 16:], 20, npix, 1, 3)
    assert torch.equal(dst[:, 16:17], src) and float(dst[:, 17:].abs().max()) == 0.0 and bool((dst[:, :16] == 9.0).all())
    dst = torch.full((npix, 20), 9.0, device='cuda')
    src = torch.randn(npix, 5, generator=g).cuda()
    lib.call('dis_copy_channels', src, 5, dst[:, 6:], 20, npix, 5, 2)
    assert torch.equal(dst[:, 6:11], src) and float(dst[:, 11:13].abs().max()) == 0.0
    assert bool((dst[:, :6] == 9.0).all()) and bool((dst[:, 13:] == 9.0).all())
    assert lib.fn('dis_copy_channels')(None, 1, None, 4, 10, 1, 0, None) != 0


def test_concat_buf_routes_gradients():
    """ops.ConcatBuf: convs write their channel range of one buffer, the joined tensor feeds the consumer, and the
    gradient ranges come back to the producers (compared with torch.cat on the same values)"""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(9)
    n, h, w = 2, 12, 10
    x = torch.randn(n, h, w, 8, generator=g).cuda().requires_grad_(True)
    w1 = (torch.randn(16, 8, 3, 3, generator=g) * 0.2).cuda().requires_grad_(True)
    w2 = (torch.randn(8, 8, 3, 3, generator=g) * 0.2).cuda().requires_grad_(True)
    w3 = (torch.randn(4, 25, 3, 3, generator=g) * 0.2).cuda().requires_grad_(True)
    d = torch.randn(n, h, w, 1, generator=g).cuda().requires_grad_(True)

    def run(inplace):
        for t in (x, w1, w2, w3, d):
            t.grad = None
        if inplace:
            cb = ops.ConcatBuf(n, h, w, 25, x.device)
            a = ops.convg(x, w1, None, 1, 1, ops.ACT_RELU, out=cb.slot(0, 16))
            b = ops.convg(x, w2, None, 1, 1, ops.ACT_RELU, out=cb.slot(16, 8))
            dd = ops.write_channels(d, cb.slot(24, 1), True)
            cat = cb.joined([(a, 0), (b, 16), (dd, 24)])
        else:
            a = ops.convg(x, w1, None, 1, 1, ops.ACT_RELU)
            b = ops.convg(x, w2, None, 1, 1, ops.ACT_RELU)
            cat = torch.cat([a, b, d, torch.zeros(n, h, w, 3, device=x.device)], dim=3)
        y = ops.convg(cat, w3, None, 1, 1, ops.ACT_NONE)
        (y * y).sum().backward()
        return y.detach().clone(), [t.grad.clone() for t in (x, w1, w2, w3, d)]

    y0, g0 = run(False)
    y1, g1 = run(True)
    assert relerr(y1, y0) < 1e-6
    for a, b in zip(g1, g0):
        assert relerr(a, b) < 1e-5
