"""The bf16 convolution family (csrc/conv_bf16.hip: BASELINE config 2) BIT FOR BIT against float64, on small-integer operands.

tests/test_sf_bf16_gpu.py holds these kernels to the bars real-valued data forces (4.7e-3 .. 1e-2 of the largest entry: the output
is rounded to 8 bits) - a dropped border tap, a wrong split-K stage boundary, a missing last 8-channel chunk or a lost pixel row
of a ragged tile all stay below them.  Here the operands are small integers (tests/int_conv_ref.py): bf16 x bf16 products are exact,
every fp32 partial sum is an integer far below 2^24 in any order, every result is an integer of magnitude <= 256 and therefore
exact in bf16.  So y, gx, gw and gb must EQUAL the float64 reference (torch.equal), and any lost, doubled or misplaced term is a
difference of at least 1.  The method rests on the bf16 MFMA's fp32 accumulation being exact for integer partial sums below 2^24:
a failure with NON-integer differences would mean that assumption failed, not that a tolerance is missing.

Every case pins the kernel it is meant to reach by the tag the dispatcher reports (lib.profile_start / profile_stop), so a routing
change that leaves a branch uncovered fails here.  The DIS_CONVB_* switches are read once per process: branches are selected by
shape only.  The only non-zero bars in this file are the SELU ones of the element-wise helpers and the sigmoid head; each is
derived where it is asserted."""
import time

import pytest
import torch
import torch.nn.functional as F

from tests import int_conv_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _diff(name, got, exp):
    """None if got == exp in every element, else a message with the count and the first few (index, got, expected)"""
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    if got.shape != exp.shape:
        return f'{name}: shape {tuple(got.shape)} != {tuple(exp.shape)}'
    if torch.equal(got, exp):
        return None
    bad = (got != exp).nonzero()
    d = (got - exp)[got != exp]
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in bad[:6]]
    whole = bool((d == d.round()).all())
    return (f'{name}: {bad.shape[0]} of {exp.numel()} differ (differences are {"integers" if whole else "NOT all integers"}, '
            f'largest {float(d.abs().max())}); first (index, got, expected): {first}')


def _recorded(fn_):
    """run fn_ under lib's per-call recorder -> (result, [(entry point, kernel tag)])"""
    from depthinspace_amd import lib
    lib.profile_start()
    out = fn_()
    return out, [(name, tag) for (name, _, _, tag, _) in lib.profile_stop()]


def _tags(rec, entry):
    return [t for n, t in rec if n == entry]


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_convb_equals_fp64_on_integers(cid):
    from depthinspace_amd import ops
    c = R.CASES[R.CASE_IDS.index(cid)]
    r = R.reference(cid)
    assert r.y_bound <= R.BOUND and r.gx_bound <= R.BOUND, (r.y_bound, r.gx_bound)   # a condition on the inputs, checked first
    act = ops.ACT_RELU if c.relu else ops.ACT_NONE
    oh, ow = R.out_hw(c)
    t0 = time.time()
    xp = R.nhwc_padded(r.x, c.cin_mem)
    xd = (xp.float() if c.x_fp32 else xp.to(BF)).cuda().requires_grad_(not c.x_fp32)
    wd, bd = r.w.float().cuda().requires_grad_(True), r.b.float().cuda().requires_grad_(True)
    if c.transposed:
        yd, rec_f = _recorded(lambda: ops.convg_transposed(xd, wd, bd, (oh, ow), 1, act, dtype=BF))
    else:
        yd, rec_f = _recorded(lambda: ops.convg(xd, wd, bd, c.stride, (c.k - 1) // 2, act, need_dgrad=not c.x_fp32, dtype=BF))
    assert yd.dtype == BF and tuple(yd.shape) == (c.n, oh, ow, c.cout)
    god = r.go.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    _, rec_b = _recorded(lambda: yd.backward(god))
    torch.cuda.synchronize()
    spent = time.time() - t0
    print(f'{cid}: forward {rec_f}\n{cid}: backward {rec_b}\n{cid}: device part {spent:.2f} s')
    bad = []
    # ---- routing ----
    tf = _tags(rec_f, 'dis_convb_run')
    if len(tf) != 1 or c.fwd not in tf[0]:
        bad.append(f'forward ran {tf}, expected one launch tagged "{c.fwd}"')
    names_b = [n for n, _ in rec_b]
    td = _tags(rec_b, 'dis_convb_run')
    if c.x_fp32:
        # fp32 network input: no input gradient, fp32 pre-activation gradient, one-pass fp32 weight / bias gradient
        if td or 'dis_convb_wgrad' in names_b or 'dis_act_bwd_bf16_f32' not in names_b:
            bad.append(f'backward of an fp32-input layer ran {rec_b}')
    else:
        if len(td) != 1 or (c.dgrad is not None and c.dgrad not in td[0]):
            bad.append(f'input gradient ran {td}, expected one call tagged "{c.dgrad}"')
        tw = _tags(rec_b, 'dis_convb_wgrad')
        if tw != [c.wgrad]:
            bad.append(f'weight gradient ran {tw}, expected ["{c.wgrad}"]')
        acts = [n for n in names_b if n.startswith('dis_act_bwd_bf16')]
        if c.relu:
            want = ['dis_act_bwd_bf16_bias'] if 256 % (c.cout // 4) == 0 else ['dis_act_bwd_bf16']
            if acts != want or (('dis_colsum_bf16' in names_b) != (want == ['dis_act_bwd_bf16'])):
                bad.append(f'activation / bias gradient ran {names_b}, expected {want}')
        elif acts or 'dis_colsum_bf16' not in names_b:   # ACT_NONE on a dense gy: gpre = gy, bias gradient by dis_colsum_bf16
            bad.append(f'ACT_NONE backward ran {names_b}')
    # ---- values: equal, not close ----
    bad.append(_diff('y', yd.float().permute(0, 3, 1, 2), r.y))
    bad.append(_diff('gw', wd.grad, r.gw))
    bad.append(_diff('gb', bd.grad, r.gb))
    if not c.x_fp32:
        assert xd.grad.dtype == BF
        gx = xd.grad.float()
        bad.append(_diff('gx', gx[..., :c.cin_w].permute(0, 3, 1, 2), r.gx))
        if c.cin_mem > c.cin_w and float(gx[..., c.cin_w:].abs().max()) != 0.0:
            bad.append(f'gx padding lanes: largest {float(gx[..., c.cin_w:].abs().max())}, expected exactly 0')
    else:
        assert xd.grad is None
    bad = [b for b in bad if b]
    for b in bad:
        print(f'{cid}: {b}')
    assert not bad, bad
    assert spent < 10.0, spent   # (the budget of a case's device part: the largest, big_tiles, is 6 images of 32 x 31 x 1024 channels)


@pytest.mark.parametrize('cin,cout,ldy,relu', [(32, 20, 24, True), (64, 68, 72, False)])
def test_convb_partial_cout_block(cin, cout, ldy, relu):
    """A cout that is a multiple of 4 but not of 8 (a 32-wide block holding 20 channels; a second 64-wide block holding 4): ops.convg
    only takes multiples of 8 for bf16 storage, so the forward runs through ops._convb_run into a channel range of a wider buffer;
    the lanes behind the range keep their bits."""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    n, h, w, k = 2, 9, 13, 3
    x = R.sparse_ints(g, n, cin, h, w, R.m_of(cin, k))
    wt, b = R.dense_ints(g, (cout, cin, k, k), -2, 2), R.dense_ints(g, (cout,), -8, 8)
    y = F.conv2d(x, wt, b, padding=1)
    y = F.relu(y) if relu else y
    assert float(F.conv2d(x.abs(), wt.abs(), b.abs(), padding=1).max()) <= R.BOUND
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    buf = torch.full((n, h, w, ldy), 9.0, dtype=BF, device='cuda')
    _, rec = _recorded(lambda: ops._convb_run(ops.CONVG_CONV, xd, wt.float().cuda(), b.float().cuda(), buf[..., :cout], n, h, w, cin, cin,
                                              h, w, cout, cout, k, 1, 1, ops.ACT_RELU if relu else ops.ACT_NONE))
    assert all(R.STREAM in t for t in _tags(rec, 'dis_convb_run')) and len(rec) == 1, rec
    msg = _diff('y', buf[..., :cout].float().permute(0, 3, 1, 2), y)
    assert msg is None, msg
    assert bool((buf[..., cout:].view(torch.int16) == torch.tensor(9.0, dtype=BF).view(torch.int16).item()).all())


# ---------------------------------------------------------------------------------------------------------------------
# the bf16 disparity head (ops._HeadStream on a bf16 x): its three convolution pieces on their own, exactly
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,h,w', [(16, 13, 17), (32, 13, 17), (64, 13, 17), (128, 13, 17), (24, 13, 17), (64, 32, 33)])
def test_convb_head_pieces_equal_fp64_on_integers(cin, h, w):
    """ops._convb_run / ops._convb_wgrad called exactly as _head_stream_fwd / _head_stream_bwd call them: the one-channel fp32
    pre-activation, the input gradient from a 4-lane fp32 buffer with one real channel, and the head weight gradient
    (stream_head_wgrad_kernel for cin in {16, 32, 64, 128}; cin = 24 has no head instance and runs the generic
    stream_wgrad_kernel with a bf16 x and an fp32 gradient).  32 x 33 = 1056 positions: the halo form with an fp32 y / an fp32 x."""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin + h)
    n, k = 2, 3
    x = R.sparse_ints(g, n, cin, h, w, R.m_of(cin, k)).requires_grad_(True)
    wt = R.dense_ints(g, (1, cin, k, k), -2, 2).requires_grad_(True)
    b = R.dense_ints(g, (1,), -8, 8)
    go = R.sparse_ints(g, n, 1, h, w, 1)              # one channel: every pixel holds +-1 or +-2
    pre = F.conv2d(x, wt, b, padding=1)
    pre.backward(go)
    assert float(F.conv2d(x.detach().abs(), wt.detach().abs(), b.abs(), padding=1).max()) <= R.BOUND
    assert float(x.grad.abs().max()) <= 9 * 2 * 2 <= R.BOUND
    halo = h * w >= 1024
    xd = x.detach().permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    wd, bd = wt.detach().float().cuda(), b.float().cuda()
    # forward, as _head_stream_fwd
    yd = torch.empty((n, 1, h, w), dtype=torch.float32, device='cuda')
    _, rec = _recorded(lambda: ops._convb_run(ops.CONVG_CONV, xd, wd, bd, yd.view(n, h, w, 1), n, h, w, cin, cin, h, w, 1, 1, k, 1,
                                              k // 2, ops.ACT_NONE))
    assert len(rec) == 1 and (R.HALO if halo else R.STREAM) in rec[0][1], rec
    msg = _diff('pre-activation', yd, pre)
    assert msg is None, msg
    # input gradient, as _head_stream_bwd
    gpre4 = torch.zeros((n, h, w, 4), dtype=torch.float32, device='cuda')
    gpre4[..., 0] = go[:, 0].float().cuda()
    gx = torch.full_like(xd, 9.0)
    _, rec = _recorded(lambda: ops._convb_run(ops.CONVG_CONV_DGRAD, gpre4, wd, None, gx, n, h, w, 4, 1, h, w, cin, cin, k, 1, k // 2,
                                              ops.ACT_NONE))
    assert len(rec) == 1 and (R.HALO if halo else R.STREAM) in rec[0][1], rec
    msg = _diff('gx', gx.float().permute(0, 3, 1, 2), x.grad)
    assert msg is None, msg
    # weight gradient
    gw = torch.full((1, cin, k, k), 9.0, dtype=torch.float32, device='cuda')
    _, rec = _recorded(lambda: ops._convb_wgrad(xd, h, w, cin, cin, gpre4, h, w, 4, 1, gw, n, k, 1, k // 2))
    tag = R.WGRAD_HEAD if cin in (16, 32, 64, 128) else R.WGRAD_GENERIC    # (an fp32 gradient never takes the slice-pair form)
    assert rec == [('dis_convb_wgrad', tag)], rec
    msg = _diff('gw', gw, wt.grad)
    assert msg is None, msg


@pytest.mark.parametrize('cin,alpha', [(128, 16.0), (64, 32.0), (32, 64.0), (16, 128.0)])
def test_disp_head_g_bf16_vs_fp64(cin, alpha):
    """ops.disp_head_g on a bf16 feature map (ops._HeadStream) against float64, the shapes of test_convg_head_fwd_bwd.  Operands that
    are exact in bf16 (integers x, multiples of 1/16 in the weights), so that the pre-activation is exact and only the sigmoid's
    fp32 evaluation separates y from float64: the fp32 twin's bar, 2e-5 of the largest entry.
    Gradients.  gw, gb: x is exact, the pre-activation gradient stays fp32 (stream_head_wgrad_kernel reads it unrounded), fp32
    sums: the fp32 twin's 5e-5 of the largest entry.  gx is a bf16 tensor computed from the fp32 pre-activation gradient, which the
    kernel rounds to bf16 when it stages it: element by element
        |gx - ref| <= 2^-8 * convT(|gpre|, |w|)     (each gpre rounded to nearest, 8 significant bits: unit roundoff 2^-8)
                    + 2^-8 * |ref|                  (the result rounded to bf16)
                    + 1e-4 * convT(|gpre|, |w|)     (gpre comes from the kernel's own fp32 y: 2e-5, and fp32 sums; generous)."""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(cin)
    n, h, w = 2, 13, 17
    x = R.sparse_ints(g, n, cin, h, w, 6)
    wt = R.dense_ints(g, (1, cin, 3, 3), -2, 2) / 16
    b = 3.0 + R.dense_ints(g, (1,), -4, 4) / 4
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = F.conv2d(xr, wr, br, padding=1)
    y = alpha * torch.sigmoid(pre - 3)
    go = torch.randn(y.shape, generator=g).double()
    y.backward(go)
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda().requires_grad_(True)
    wd, bd = wt.float().cuda().requires_grad_(True), b.float().cuda().requires_grad_(True)
    yd = ops.disp_head_g(xd, wd, bd, alpha, 3.0)
    assert yd.dtype == torch.float32 and tuple(yd.shape) == (n, 1, h, w)

    def relerr(a, ref):
        return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max())
    assert relerr(yd, y.detach()) < 2e-5
    yd.backward(go.float().cuda())
    assert relerr(wd.grad, wr.grad) < 5e-5
    assert relerr(bd.grad, br.grad) < 5e-5
    s = torch.sigmoid(pre.detach() - 3)
    gpre = go * alpha * s * (1 - s)
    l1 = F.conv_transpose2d(gpre.abs(), wt.abs(), padding=1)
    bar = 2.0 ** -8 * l1 + 2.0 ** -8 * xr.grad.abs() + 1e-4 * l1
    err = (xd.grad.float().cpu().double().permute(0, 3, 1, 2) - xr.grad).abs()
    assert xd.grad.dtype == BF and bool((err <= bar).all()), float((err - bar).max())


# ---------------------------------------------------------------------------------------------------------------------
# the bf16 element-wise helpers, on channel ranges of wider buffers
# ---------------------------------------------------------------------------------------------------------------------
SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
CSB_BLOCKS = 1024   # conv_bf16.hip: block partials of dis_act_bwd_bf16_bias / dis_colsum_bf16


def _bf16_ulp(t):
    """the spacing of bf16 numbers at |t| (8 significant bits), float64"""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


# c, ldg, goff, ldy, yoff, npix.  Channels per thread of the _bias kernel: 8 needs c, ldg, ldy multiples of 8, 16-byte aligned ranges
# and 256 % (c / 8) == 0, else 4 (256 % (c / 4) == 0), else the entry point declines.  rows = pixels per block = 256 / (c / V).
ACT_SHAPES = [
    (24, 40, 8, 32, 4, 1000, None),                 # 4 per thread (act_bwd / _f32); 256 % 6 != 0: the _bias entry declines
    (32, 40, 4, 40, 8, 1000, 4),                    # 4 per thread in the _bias kernel (gy range only 8-byte aligned)
    (64, 64, 0, 64, 0, 1000, 8),                    # 8 per thread
    (8, 8, 0, 16, 8, 777, 8),                       # one 8-channel vector per pixel, rows = 256
    (64, 64, 0, 64, 0, 1, 8),                       # one pixel
    (16, 24, 4, 16, 0, 1, 4),
    (64, 64, 0, 64, 0, CSB_BLOCKS * 32 + 37, 8),    # rows = 32: just past CSB_BLOCKS * rows, 37 blocks walk a second pixel
    (32, 40, 4, 40, 8, CSB_BLOCKS * 32 + 37, 4),
    (20, 24, 4, 24, 0, 500, None),                  # 256 % 5 != 0: the _bias entry declines
]


@pytest.mark.parametrize('c,ldg,goff,ldy,yoff,npix,vec', ACT_SHAPES)
def test_act_bwd_bf16_helpers(c, ldg, goff, ldy, yoff, npix, vec):
    """dis_act_bwd_bf16 / _f32 / _bias: gpre = gy * act'(y) on channel ranges, bf16 or fp32 result, with the bias gradient (column
    sums of the unrounded gpre).  Integer gy under ReLU and ACT_NONE: everything exact, bias sums included (integers < 2^24).
    SELU on real-valued data: gpre within one bf16 ulp of the float64 product; the bias sum within 1e-5 * sum|gpre| of the float64
    sum: a thread adds at most ceil(npix / (1024 * rows)) <= 2 terms here, a block's fold adds its `rows` <= 256 fp32 partials
    one after the other, the blocks are summed in float64.  That is a chain of at most a few hundred fp32 additions at 2^-24 each:
    1.5e-5 of sum|gpre| if every rounding error had the same sign, ~ sqrt(256) * 2^-24 = 1e-6 for errors of random sign; the bar
    sits between the two."""
    from depthinspace_amd import lib, ops
    g = torch.Generator().manual_seed(c * 31 + npix % 1000)
    for act in (ops.ACT_RELU, ops.ACT_NONE, ops.ACT_SELU):
        if act == ops.ACT_SELU:
            gyw = torch.randn(npix, ldg, generator=g).to(BF)
            yw = F.selu(torch.randn(npix, ldy, generator=g).double()).clamp_min(-1.5).to(BF)   # (SELU outputs; away from the zero of y + scale * alpha)
        else:
            gyw = torch.randint(-3, 4, (npix, ldg), generator=g).to(BF)
            yw = torch.randn(npix, ldy, generator=g).to(BF)
            yw[::7] = 0.0                                                                        # (y == 0: gradient 0 under ReLU)
        gyd, ywd = gyw.cuda(), yw.cuda()
        gy, y = gyd[:, goff:goff + c], ywd[:, yoff:yoff + c]
        g64, y64 = gyw[:, goff:goff + c].double(), yw[:, yoff:yoff + c].double()
        if act == ops.ACT_RELU:
            ref = g64 * (y64 > 0)
        elif act == ops.ACT_NONE:
            ref = g64
        else:
            ref = g64 * torch.where(y64 > 0, torch.full_like(y64, SELU_SCALE), y64 + SELU_SCALE * SELU_ALPHA)
        yarg = y if act != ops.ACT_NONE else None
        gp = torch.full((npix, c), 9.0, dtype=BF, device='cuda')
        lib.call('dis_act_bwd_bf16', gy, ldg, yarg, ldy, gp, act, npix, c)
        gp32 = torch.full((npix, c), 9.0, dtype=torch.float32, device='cuda')
        lib.call('dis_act_bwd_bf16_f32', gy, ldg, yarg, ldy, gp32, act, npix, c)
        outs = [('dis_act_bwd_bf16', gp), ('dis_act_bwd_bf16_f32', gp32)]
        gb = None
        gpb = torch.full((npix, c), 9.0, dtype=BF, device='cuda')
        gbd = torch.full((c,), 9.0, dtype=torch.float32, device='cuda')
        ws = torch.empty(lib.fn('dis_colsum_bf16_workspace')(c), dtype=torch.float32, device='cuda')
        if vec is None:
            with pytest.raises(lib.DisHipError):
                lib.call('dis_act_bwd_bf16_bias', gy, ldg, yarg, ldy, gpb, act, npix, c, gbd, ws)
        else:
            v8 = c % 8 == 0 and ldg % 8 == 0 and ldy % 8 == 0 and gy.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and 256 % (c // 8) == 0
            assert (8 if v8 else 4) == vec          # (the shape reaches the instance it is listed for)
            lib.call('dis_act_bwd_bf16_bias', gy, ldg, yarg, ldy, gpb, act, npix, c, gbd, ws)
            outs.append(('dis_act_bwd_bf16_bias', gpb))
            gb = gbd.double().cpu()
        for name, t in outs:
            got = t.double().cpu()
            if act != ops.ACT_SELU:
                msg = _diff(f'{name} act {act}', got, ref)
                assert msg is None, msg
            elif t.dtype == BF:
                assert bool(((got - ref).abs() <= _bf16_ulp(ref)).all()), (name, float(((got - ref).abs() / _bf16_ulp(ref)).max()))
            else:
                # fp32 result: two fp32 roundings (y + scale * alpha, the product: 2^-24 each) and the fp32 constants themselves
                # (scale * alpha = 1.758 and scale, off by at most 2^-24 of their value: <= 2^-23 * |gy| in the product)
                assert bool(((got - ref).abs() <= 2.0 ** -22 * ref.abs() + 2.0 ** -23 * g64.abs()).all()), name
        if gb is not None:
            if act != ops.ACT_SELU:
                msg = _diff(f'bias gradient act {act}', gb, ref.sum(0))
                assert msg is None, msg
            else:
                assert bool(((gb - ref.sum(0)).abs() <= 1e-5 * ref.abs().sum(0)).all())


@pytest.mark.parametrize('src_bf16', [False, True])
@pytest.mark.parametrize('c,czero', [(1, 0), (1, 3), (5, 0), (5, 2)])
def test_copy_channels_bf16(src_bf16, c, czero):
    """dis_copy_channels_bf16: an fp32 or bf16 source into a channel range of a bf16 buffer, with or without a zero tail; the
    neighbouring lanes keep their BITS; fp32 values land on round-to-nearest-even (tensor.to(bfloat16)), ties included."""
    from depthinspace_amd import lib
    g = torch.Generator().manual_seed(7 + c + czero)
    npix, ldd, off = 1000, 24, 8
    src = torch.randn(npix, c, generator=g)
    # ties of the rounding: 1 + 2^-8 -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6, just above / below a tie, a negative tie
    src[:6, 0] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, -(1 + 2.0 ** -8), 0.0])
    if src_bf16:
        src = src.to(BF)
    want = src.to(BF)
    sentinel = torch.tensor(-7.5, dtype=BF)
    dst = torch.full((npix, ldd), -7.5, dtype=BF, device='cuda')
    srcd = src.cuda()
    lib.call('dis_copy_channels_bf16', srcd, 1 if src_bf16 else 0, c, dst[:, off:], ldd, npix, c, czero)
    bits = dst.cpu().view(torch.int16)
    assert torch.equal(bits[:, off:off + c], want.view(torch.int16))
    assert bool((bits[:, off + c:off + c + czero] == 0).all())                     # (+0.0, not -0.0)
    sb = sentinel.view(torch.int16).item()
    assert bool((bits[:, :off] == sb).all()) and bool((bits[:, off + c + czero:] == sb).all())
    assert lib.fn('dis_copy_channels_bf16')(None, 0, 1, None, 4, 10, 1, 0, None) != 0


@pytest.mark.parametrize('c,ldg,goff,npix', [(24, 40, 8, 1000), (300, 304, 0, 513), (1, 8, 3, 1000), (24, 40, 8, 3), (24, 40, 8, 70000)])
def test_colsum_bf16(c, ldg, goff, npix):
    """dis_colsum_bf16 on integers (exact): a c that does not divide 256, two passes of the 256-channel loop, one channel at an odd
    offset, fewer pixels than a block has rows, more than one block (70 000 pixels: 274 blocks)."""
    from depthinspace_amd import lib
    g = torch.Generator().manual_seed(c + npix)
    G = torch.randint(-2, 3, (npix, ldg), generator=g).to(BF)
    out = torch.full((c,), 9.0, dtype=torch.float32, device='cuda')
    ws = torch.empty(lib.fn('dis_colsum_bf16_workspace')(c), dtype=torch.float32, device='cuda')
    lib.call('dis_colsum_bf16', G.cuda(), ldg, goff, npix, c, out, ws)
    msg = _diff('column sums', out, G[:, goff:goff + c].double().sum(0))
    assert msg is None, msg
