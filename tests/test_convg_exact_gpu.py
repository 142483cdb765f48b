"""The fp32-storage streaming convolutions (csrc/conv_gen.hip behind ops.convg / ops.convg_transposed, with the channel slices, the
one-pass and slice-pair weight gradients of conv2d.hip / conv_f16x2.hip and the generic one of conv_stream_wgrad.hip) BIT FOR BIT
against float64, on wide-integer operands.

tests/test_sf_gpu.py holds these kernels to 2e-5 / 5e-5 of the largest entry.  Under the default two-term fp16 split a product is
a1 b1 + a1 b2 + a2 b1; one a2 b1 term lost at a ragged tile edge, in the last 32-channel chunk, at a split-K boundary or in one
parity phase is ~2^-12 of ONE term of up to 9216: far below those bars.  Here (tests/int_conv_f32_ref.py) the operands are dense
integers in [-2, 2] with a sprinkle of +-2049 = 2^11 + 1 placed so that no product has two wide factors: the split is exact, the
dropped a2 b2 term is identically zero, and with the asserted L1 bounds < 2^24 every fp32 partial sum is exact in any order.  So
y, gx, gw and gb must EQUAL the reference (torch.equal): a lost first-plane term is a difference of at least 1, a lost second-plane
term exactly the low part of a wide value.  A failure with NON-integer differences means the exactness premise failed (a scale that
is no power of two, a contraction, an accumulator out of range), not that a tolerance is missing: no comparison in this file has one.

Every case pins the kernel each of its calls is meant to reach by the tag the dispatcher reports (lib.profile_start / profile_stop);
for a phased call that runs as four launches the recorder keeps the LAST phase's tag.  Branches are selected by shape only - the
DIS_CONVG_* switches are not touched.  Every case runs under the default split; the cases with a split3 entry in the table also run
under conv_split('bf16x3') (convg3, the three-term slices and slice pairs)."""
import time

import pytest
import torch
import torch.nn.functional as F

from tests import int_conv_f32_ref as R
from tests.conftest import conv_split
from tests.test_convb_exact_gpu import _diff, _recorded, _tags

pytestmark = pytest.mark.gpu

FILL = 1.0e6    # lanes of the wider buffers outside the channel ranges: one of them in a sum is off by far more than any entry


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _range_of(t_nhwc, ld, off):
    """(n, h, w, c) fp32 CPU tensor -> device buffer (n, h, w, ld) with t in lanes [off, off + c) and FILL elsewhere; the channel range"""
    n, h, w, c = t_nhwc.shape
    buf = torch.full((n, h, w, ld), FILL, dtype=torch.float32)
    buf[..., off:off + c] = t_nhwc
    buf = buf.cuda()
    return buf, buf[..., off:off + c]


def _run_case(c, r, want, label):
    """one forward + backward of the case under the current split -> list of findings (empty: routed and equal)"""
    from depthinspace_amd import ops
    want_fwd, want_dgrad, want_wgrad = want
    act = ops.ACT_RELU if c.relu else ops.ACT_NONE
    oh, ow = R.out_hw(c)
    t0 = time.time()
    xp = R.nhwc_padded(r.x, c.cin_mem).float()
    gop = r.go.permute(0, 2, 3, 1).contiguous().float()
    out, cb = None, None
    if c.slot:
        ldx, xoff, ldy, yoff, ldg, goff = c.slot
        xbuf, xr = _range_of(xp, ldx, xoff)
        xd = xr.detach().requires_grad_(True)          # (a leaf that shares the buffer's memory)
        gbuf, god = _range_of(gop, ldg, goff)
        cb = ops.ConcatBuf(c.n, oh, ow, ldy, 'cuda')
        cb.buf.fill_(FILL)
        out = cb.slot(yoff, c.cout)
        x0, g0 = _bits(xbuf).clone(), _bits(gbuf).clone()
    else:
        xd = xp.cuda().requires_grad_(c.need_dgrad)
        god = gop.cuda()
    wd, bd = r.w.float().cuda().requires_grad_(True), r.b.float().cuda().requires_grad_(True)
    if c.transposed:
        yd, rec_f = _recorded(lambda: ops.convg_transposed(xd, wd, bd, (oh, ow), 1, act, out=out, dtype=torch.float32))
    else:
        yd, rec_f = _recorded(lambda: ops.convg(xd, wd, bd, c.stride, (c.k - 1) // 2, act, need_dgrad=c.need_dgrad, out=out,
                                                dtype=torch.float32))
    assert yd.dtype == torch.float32 and tuple(yd.shape) == (c.n, oh, ow, c.cout)
    _, rec_b = _recorded(lambda: yd.backward(god))
    torch.cuda.synchronize()
    spent = time.time() - t0
    print(f'{label}: forward {rec_f}\n{label}: backward {rec_b}\n{label}: device part {spent:.2f} s')
    bad = []
    # ---- routing ----
    tf = _tags(rec_f, 'dis_convg_run')
    if tf != [want_fwd]:
        bad.append(f'forward ran {tf}, expected ["{want_fwd}"]')
    td = _tags(rec_b, 'dis_convg_run')
    if td != ([want_dgrad] if c.need_dgrad else []):
        bad.append(f'input gradient ran {td}, expected ["{want_dgrad}"]')
    names_b = [n for n, _ in rec_b]
    tw = [(n, t) for n, t in rec_b if n in ('dis_convg_wgrad', 'dis_conv2d_wgrad', 'dis_conv2d_wgrad_bf16x3')]
    if tw != [want_wgrad]:
        bad.append(f'weight gradient ran {tw}, expected [{want_wgrad}]')
    # bias gradient: out of the one-pass weight-gradient kernel; else with the pre-activation gradient (dis_act_bwd_ld_bias) when
    # there is one to form (an activation, or a gy that is a channel range) and 256 % (cout / 4) == 0; else dis_colsum
    if want_wgrad[0] != 'dis_convg_wgrad':
        want_bias = []
    elif (c.relu or c.slot) and 256 % (c.cout // 4) == 0:
        want_bias = ['dis_act_bwd_ld_bias']
    else:
        want_bias = ['dis_colsum']
    got_bias = [n for n in names_b if n in ('dis_act_bwd_ld_bias', 'dis_colsum')]
    if got_bias != want_bias:
        bad.append(f'bias gradient ran {got_bias} of {names_b}, expected {want_bias}')
    # ---- values: equal, not close ----
    bad.append(_diff('y', yd.permute(0, 3, 1, 2), r.y))
    bad.append(_diff('gw', wd.grad, r.gw))
    bad.append(_diff('gb', bd.grad, r.gb))
    if c.need_dgrad:
        gx = xd.grad
        bad.append(_diff('gx', gx[..., :c.cin_w].permute(0, 3, 1, 2), r.gx))
        if c.cin_mem > c.cin_w and float(gx[..., c.cin_w:].abs().max()) != 0.0:
            bad.append(f'gx padding lanes: largest {float(gx[..., c.cin_w:].abs().max())}, expected exactly 0')
    else:
        assert xd.grad is None
    if c.slot:   # the foreign lanes keep their bits
        if not torch.equal(_bits(xbuf), x0) or not torch.equal(_bits(gbuf), g0):
            bad.append('the buffer x / gy was read from has changed')
        lanes = torch.ones(ldy, dtype=torch.bool)
        lanes[yoff:yoff + c.cout] = False
        fill_bits = torch.tensor(FILL, dtype=torch.float32).view(torch.int32).item()
        if not bool((_bits(cb.buf)[..., lanes.cuda()] == fill_bits).all()):
            bad.append('lanes of the output buffer outside the slot have changed')
    if spent >= 10.0:
        bad.append(f'device part took {spent:.1f} s')
    return [f'{label}: {b}' for b in bad if b]


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_convg_equals_fp64_on_wide_integers(cid):
    c = R.case(cid)
    r = R.reference(cid)
    print(f'{cid}: L1 bounds y {r.y_bound:.0f} gx {r.gx_bound:.0f} gw/gb {r.gw_bound:.0f}; host reference in {r.y.dtype}')
    assert max(r.y_bound, r.gx_bound, r.gw_bound) < R.BOUND, (r.y_bound, r.gx_bound, r.gw_bound)   # conditions on the inputs, first
    bad = _run_case(c, r, (c.fwd, c.dgrad, c.wgrad), cid)
    if c.split3:
        with conv_split('bf16x3'):
            bad += _run_case(c, r, c.split3, cid + ' bf16x3')
    for b in bad:
        print(b)
    assert not bad, bad


@pytest.mark.parametrize('cin,h,w', [(64, 13, 17), (128, 13, 17), (64, 32, 33)])
def test_convg_head_pieces_equal_fp64_on_wide_integers(cin, h, w):
    """ops._convg_run called exactly as _head_stream_fwd / _head_stream_bwd call it on fp32 storage: the one-channel pre-activation
    (convg2 with a 16-wide block holding one channel; 32 x 33 = 1056 positions: the halo form with a one-channel y), and the input
    gradient from a 4-lane buffer with one real channel (the tap-packed fp32 MFMA kernel).  One output channel leaves no even / odd
    freedom: the forward's weight is wide at odd input channels (x: even ones, image 0); the input gradient takes a narrow weight
    and a gradient that is wide in image 1.  (The fp32 head weight gradient: tests/test_stream_wgrad_exact_gpu.py.)"""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(1000 * cin + h)
    n, k = 2, 3
    odd = (torch.arange(cin) % 2 == 1).view(1, cin, 1, 1)
    x = R.wide_ints(g, (n, cin, h, w), -2, 2, R.act_eligible(n, cin, 0), 0.1, [(0, cin - 2, h - 1, w - 1)])
    wf = R.wide_ints(g, (1, cin, k, k), -2, 2, odd, 0.1, [(0, cin - 1, 0, 0), (0, cin - 1, k - 1, k - 1)])
    wn = R.dense_ints(g, (1, cin, k, k), -2, 2)
    b = R.dense_ints(g, (1,), -8, 8)
    go = R.wide_ints(g, (n, 1, h, w), -2, 2, (torch.arange(n) == 1).view(n, 1, 1, 1), 0.1, [(1, 0, h - 1, w - 1)])
    pre = F.conv2d(x, wf, b, padding=1)
    gx_ref = F.conv_transpose2d(go, wn, padding=1)
    assert float(F.conv2d(x.abs(), wf.abs(), b.abs(), padding=1).max()) < R.BOUND
    assert float(F.conv_transpose2d(go.abs(), wn.abs(), padding=1).max()) < R.BOUND
    assert not bool(((x.abs() == R.WIDE).any(dim=(0, 2, 3)) & (wf.abs() == R.WIDE).any(dim=(0, 2, 3))).any())   # never wide x wide
    halo = h * w >= 1024
    xd = x.permute(0, 2, 3, 1).contiguous().float().cuda()
    # forward, as _head_stream_fwd
    yd = torch.full((n, 1, h, w), 9.0, dtype=torch.float32, device='cuda')
    _, rec = _recorded(lambda: ops._convg_run(ops.CONVG_CONV, xd, wf.float().cuda(), b.float().cuda(), yd.view(n, h, w, 1), n, h, w, cin,
                                              cin, h, w, 1, 1, k, 1, k // 2, ops.ACT_NONE))
    print(f'head {cin} {h}x{w}: forward {rec}')
    assert rec == [('dis_convg_run', R.H2_RES if halo else R.G2)], rec
    msg = _diff('pre-activation', yd, pre)
    assert msg is None, msg
    # input gradient, as _head_stream_bwd
    gpre4 = torch.zeros((n, h, w, 4), dtype=torch.float32)
    gpre4[..., 0] = go[:, 0].float()
    gpre4 = gpre4.cuda()
    gx = torch.full_like(xd, 9.0)
    _, rec = _recorded(lambda: ops._convg_run(ops.CONVG_CONV_DGRAD, gpre4, wn.float().cuda(), None, gx, n, h, w, 4, 1, h, w, cin, cin, k,
                                              1, k // 2, ops.ACT_NONE))
    print(f'head {cin} {h}x{w}: input gradient {rec}')
    assert rec == [('dis_convg_run', R.FP32)], rec
    msg = _diff('gx', gx.permute(0, 3, 1, 2), gx_ref)
    assert msg is None, msg
