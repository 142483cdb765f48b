"""dis_conv2d_bwd_fused_f16x2_c16 (csrc/conv_bwd_fused_c16.hip): the input gradient and the weight gradient of a 3x3 conv with 16
channels on a side in ONE launch, against the two launches it replaces and against fp64.

Reference semantics: torch.nn.Conv2d's backward inside FuseNet's 16-channel ResNetBlocks and stem convs
(model/multi_frame_networks.py).  Bars (tests/test_bwd_fused_gpu.py's): gx BIT-identical to the unfused input-gradient launch, the
stored operand bit-identical where the form stores it, the GroupNorm-backward channel sums within 1e-6, grad_w / grad_b within 1e-6 of
the largest entry of the fp64 result and no further from fp64 than twice the error of the two launches replaced."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (cin, cout) pairs with a kernel and the forms each ships with
FORMS = ['plain', 'plain_accum', 'plain_act', 'plain_act_accum', 'coef', 'coef_act', 'coef_sums_xgn', 'coef_act_sums_xgn',
         'coef_sums_xgn_store', 'coef_act_accum', 'two_consumer', 'chain']
PAIRS = [(16, 16)]
# ragged tiles in both directions, a one-tile-high map, more than one sample, a map smaller than the grid
SHAPES = [(3, 37, 29), (2, 64, 48), (2, 16, 250), (1, 20, 20)]
SELU_S, SELU_A = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def _fp64_wgrad(x, gpre):
    xn = x.permute(0, 3, 1, 2).double()
    gn = gpre.permute(0, 3, 1, 2).double()
    gw = torch.nn.grad.conv2d_weight(xn, (gn.shape[1], xn.shape[1], 3, 3), gn, padding=1)
    return gw, gn.sum(dim=(0, 2, 3))


def _fused(L, g, q, coef, in_act, gpre, wt, gx, accum, ab_x, act_y, ab, slots, x, xg, gw, gb, n, h, w, stride=0):
    cout, cin = wt.shape[0], wt.shape[1]
    ws = torch.empty(L.fn('dis_conv2d_bwd_fused_c16_workspace')(cin, cout), dtype=torch.float32, device='cuda')
    return L.call_try('dis_conv2d_bwd_fused_f16x2_c16', g, q, coef, in_act, gpre, wt, cout, cin, wt.stride(0), gx, 1 if accum else 0,
                      ab_x, act_y, ab, slots, x, xg[0] if xg else None, xg[1] if xg else None, xg[2] if xg else None, 1e-5, gw, gb,
                      ws, n, h, w, stride)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n,h,w', SHAPES)
@pytest.mark.parametrize('cin,cout', PAIRS)
def test_bwd_fused_c16_matches_the_two_launches(cin, cout, form, n, h, w):
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_get_conv_split')() == 1
    S = ops.ACT_SELU
    g_ = torch.Generator().manual_seed(2000 + 7 * h + w + len(form) + cin)
    rnd = lambda *s: torch.randn(*s, generator=g_).cuda()
    coef_form = form.startswith(('coef', 'two_consumer', 'chain'))
    in_act = S if form in ('plain_act', 'plain_act_accum', 'coef_act', 'coef_act_sums_xgn', 'coef_act_accum', 'two_consumer', 'chain') else 0
    accum = form in ('plain_accum', 'plain_act_accum', 'coef_act_accum', 'two_consumer', 'chain')
    sums = 'sums' in form or form in ('two_consumer', 'chain')
    xgn = 'xgn' in form
    store = form.endswith('store')
    q = rnd(n, h, w, cout)
    if in_act:
        q = F.selu(q)
    gq = rnd(n, h, w, cout) * (1.0 + 3.0 * torch.rand(n, 1, 1, 1, generator=g_).cuda())   # per-sample magnitudes differ: the running scales move
    wt = (rnd(cout, cin, 3, 3) * 0.05).contiguous()
    x = rnd(n, h, w, cin) * 2.0 + 0.3
    if form == 'chain':
        x = F.selu(x)          # x = SELU(GroupNorm(x2) + res): the activation output the result is multiplied with
    slots_ref = L.fn('dis_conv2d_gnsums_slots')()
    slots = L.fn('dis_conv2d_bwd_fused_c16_slots')(cin, cout)
    assert slots >= slots_ref
    base = rnd(n, h, w, cin)
    coef = None
    if coef_form:
        assert cin == cout
        c = cout
        gamma = (torch.rand(c, generator=g_) + 0.5).cuda()
        st = torch.stack([q.double().sum(dim=(1, 2, 3)), (q.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
        ab0 = torch.zeros(n, slots_ref, 2, c, dtype=torch.float64, device='cuda')
        ab0[:, 0, 0] = gq.double().sum(dim=(1, 2))
        ab0[:, 0, 1] = (gq.double() * q.double()).sum(dim=(1, 2))
        coef = torch.empty(n * (c + 2) + 4 * n * c + 2, dtype=torch.float32, device='cuda')
        gg, gb_ = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
        L.call('dis_gn_bwd_coef', st, gamma, ab0, slots_ref, coef, gg, gb_, torch.zeros(2, dtype=torch.int32, device='cuda'), n, h * w, c, 1e-5)
    ab_x = act_y = None
    if form in ('coef_sums_xgn', 'coef_act_sums_xgn', 'coef_sums_xgn_store'):
        ab_x = x                       # conv2d_gn_in: the GroupNorm input of the sums IS the conv's input
    elif form == 'two_consumer':
        ab_x = rnd(n, h, w, cin)
    elif form == 'chain':
        ab_x = rnd(n, h, w, cin)
        act_y = x
    xg = None
    if xgn:
        xst = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
        xgam, xbet = (torch.rand(cin, generator=g_) + 0.5).cuda(), (torch.randn(cin, generator=g_) * 0.1).cuda()
        xg = (xst, xgam, xbet)
    # ---- the two launches replaced
    gx_ref = base.clone()
    ab_ref = torch.zeros(n * slots_ref * 2 * cin, dtype=torch.float64, device='cuda') if sums else None
    if coef_form:
        gpre_ref = torch.empty_like(gq)
        assert L.call_try('dis_conv2d_dgrad_f16x2_gnb', gq, q, coef, in_act, gpre_ref, wt, cout, cin, wt.stride(0), gx_ref,
                          1 if accum else 0, ab_x, act_y, ab_ref, n, h, w, cin)
    elif in_act:
        gpre_ref = gq * torch.where(q > 0, torch.full_like(q, SELU_S), q + SELU_S * SELU_A)
        L.call('dis_conv2d_dgrad_bf16x3_act', gq, q, in_act, wt, cout, cin, wt.stride(0), gx_ref, n, h, w, cout, cin, 1, 1 if accum else 0)
    else:
        gpre_ref = gq
        L.call('dis_conv2d_fwd_bf16x3_oihw', gq, wt, 1, cout, cin, wt.stride(0), None, gx_ref, None, n, h, w, cout, cin, 3, 1, 1,
               ops.CONV_ACCUM if accum else 0)
    wsz = L.fn('dis_conv2d_wgrad_workspace')(cin, cout, 3, 1)
    gw_ref, gb_ref = torch.empty(cout, cin, 3, 3, device='cuda'), torch.empty(cout, device='cuda')
    ws = torch.empty(wsz, dtype=torch.float32, device='cuda')
    if xgn:
        L.call('dis_conv2d_wgrad_bf16x3_gn', x, xg[0], xg[1], xg[2], 1e-5, gpre_ref, gw_ref, gb_ref, ws, n, h, w, cin, cin, cout, 3, 1, 1)
    else:
        L.call('dis_conv2d_wgrad_bf16x3', x, gpre_ref, gw_ref, gb_ref, ws, n, h, w, cin, cin, cout, 3, 1, 1)
    # ---- fp64
    x_eff = x
    if xgn:
        mean = (xg[0].view(n, 2)[:, 0] / (h * w * cin)).view(n, 1, 1, 1)
        var = (xg[0].view(n, 2)[:, 1] / (h * w * cin)).view(n, 1, 1, 1) - mean ** 2
        x_eff = ((x.double() - mean) / torch.sqrt(var + 1e-5) * xg[1].double() + xg[2].double())
    gw64, gb64 = _fp64_wgrad(x_eff, gpre_ref)
    # ---- the fused launch
    gx = base.clone()
    gpre = torch.full_like(gq, float('nan')) if store else None
    ab = torch.zeros(n * slots * 2 * cin, dtype=torch.float64, device='cuda') if sums else None
    gw, gb = torch.full((cout, cin, 3, 3), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda')
    assert _fused(L, gq, q if (coef_form or in_act) else None, coef, in_act, gpre, wt, gx, accum, ab_x, act_y, ab, slots, x, xg, gw, gb,
                  n, h, w), 'no instance for a form the step uses'
    torch.cuda.synchronize()
    assert torch.equal(gx, gx_ref), float((gx - gx_ref).abs().max())
    if store:
        assert torch.equal(gpre, gpre_ref)
    if sums:
        got, ref = ab.view(n, slots, 2, cin).sum(dim=1), ab_ref.view(n, slots_ref, 2, cin).sum(dim=1)
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), float((got - ref).abs().max())
    sw, sb = float(gw64.abs().max()), float(gb64.abs().max())
    e_new, e_old = float((gw.double() - gw64).abs().max()) / sw, float((gw_ref.double() - gw64).abs().max()) / sw
    b_new, b_old = float((gb.double() - gb64).abs().max()) / sb, float((gb_ref.double() - gb64).abs().max()) / sb
    print(form, (cin, cout), (n, h, w), 'grad_w err / largest: fused %.2e, two launches %.2e; grad_b %.2e / %.2e' % (e_new, e_old, b_new, b_old))
    assert e_new < 1e-6, (e_new, e_old)
    assert b_new < 1e-6, (b_new, b_old)
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert b_new <= 2 * b_old, (b_new, b_old)


@pytest.mark.parametrize('cin,cout', PAIRS)
def test_bwd_fused_c16_is_reproducible_and_handles_extreme_ranges(cin, cout):
    """a 1e4 outlier in one sample, a 1e-6 sample, zeros in another: the running dW exponent moves, nothing overflows, and the launch
    repeats bit for bit (fixed summation orders, no atomics)"""
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_get_conv_split')() == 1
    n, h, w = 5, 48, 40
    g_ = torch.Generator().manual_seed(77)
    gy = torch.randn(n, h, w, cout, generator=g_).cuda()
    x = torch.randn(n, h, w, cin, generator=g_).cuda()
    gy[1] *= 1e-6
    x[2] = 0.0
    gy[3, 7, 9, 5] = 1e4
    x[4, 30, 2, 11] = -3e3
    gy[0, :16, :16] = 0.0
    wt = (torch.randn(cout, cin, 3, 3, generator=g_) * 0.05).cuda()
    outs = []
    for rep in range(3):
        gx = torch.empty_like(x)
        gw, gb = torch.empty(cout, cin, 3, 3, device='cuda'), torch.empty(cout, device='cuda')
        assert _fused(L, gy, None, None, 0, None, wt, gx, False, None, None, None, 0, x, None, gw, gb, n, h, w)
        outs.append((gx, gw, gb))
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert all(torch.equal(a_, b_) for a_, b_ in zip(o, outs[0]))
    # the two launches replaced, on the same inputs: gx bit for bit, grad_w / grad_b beside them against fp64
    gx_ref = torch.empty_like(x)
    L.call('dis_conv2d_fwd_bf16x3_oihw', gy, wt, 1, cout, cin, wt.stride(0), None, gx_ref, None, n, h, w, cout, cin, 3, 1, 1, 0)
    gw_ref, gb_ref = torch.empty(cout, cin, 3, 3, device='cuda'), torch.empty(cout, device='cuda')
    ws = torch.empty(L.fn('dis_conv2d_wgrad_workspace')(cin, cout, 3, 1), dtype=torch.float32, device='cuda')
    L.call('dis_conv2d_wgrad_bf16x3', x, gy, gw_ref, gb_ref, ws, n, h, w, cin, cin, cout, 3, 1, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0][0]).all()) and torch.equal(outs[0][0], gx_ref)
    gw64, gb64 = _fp64_wgrad(x, gy)
    assert bool(torch.isfinite(outs[0][1]).all()) and bool(torch.isfinite(outs[0][2]).all())
    sw, sb = float(gw64.abs().max()), float(gb64.abs().max())
    e_new, e_old = float((outs[0][1].double() - gw64).abs().max()) / sw, float((gw_ref.double() - gw64).abs().max()) / sw
    b_new, b_old = float((outs[0][2].double() - gb64).abs().max()) / sb, float((gb_ref.double() - gb64).abs().max()) / sb
    print('range case', (cin, cout), 'grad_w %.2e (two launches %.2e), grad_b %.2e (%.2e)' % (e_new, e_old, b_new, b_old))
    assert e_new < 1e-6 and b_new < 1e-6, (e_new, b_new)
    assert e_new <= 2 * e_old and b_new <= 2 * b_old, (e_new, e_old, b_new, b_old)


@pytest.mark.parametrize('cin,cout', PAIRS)
def test_bwd_fused_c16_writes_a_slice_of_a_wider_weight_gradient(cin, cout):
    """grad_w_row_stride: the slab reduce writes the (cout, cin, 3, 3) slice of a (cout, 48, 3, 3) gradient in place (ref_conv's conv
    over a channel concatenation): the slice equals the contiguous result bit for bit, the neighbouring columns are untouched."""
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_get_conv_split')() == 1
    n, h, w = 2, 40, 56
    g_ = torch.Generator().manual_seed(5)
    gy = torch.randn(n, h, w, cout, generator=g_).cuda()
    x = torch.randn(n, h, w, cin, generator=g_).cuda()
    wt = (torch.randn(cout, cin, 3, 3, generator=g_) * 0.05).cuda()

    def run(gw, stride):
        gx, gb = torch.empty_like(x), torch.empty(cout, device='cuda')
        ok = _fused(L, gy, None, None, 0, None, wt, gx, False, None, None, None, 0, x, None, gw, gb, n, h, w, stride)
        torch.cuda.synchronize()
        return ok, gx, gb

    ref = torch.empty(cout, cin, 3, 3, device='cuda')
    ok, gx0, gb0 = run(ref, 0)
    assert ok
    wide = torch.full((cout, 48, 3, 3), 7.0, device='cuda')
    lo = 48 - cin - 8
    sl = wide[:, lo:lo + cin]
    ok, gx1, gb1 = run(sl, sl.stride(0))
    assert ok and torch.equal(gx0, gx1) and torch.equal(gb0, gb1)
    assert torch.equal(sl, ref)
    assert bool((wide[:, :lo] == 7.0).all()) and bool((wide[:, lo + cin:] == 7.0).all())
    for bad in (cin * 9 + 1, cin * 9 - 9):   # a pitch that is not whole input channels / narrower than the slice is refused
        with pytest.raises(L.DisHipError):
            run(ref, bad)


def test_bwd_fused_c16_entry_point_refuses_what_it_lacks():
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_conv2d_bwd_fused_c16_workspace')(32, 32) < 0 and L.fn('dis_conv2d_bwd_fused_c16_workspace')(8, 16) < 0
    n, h, w = 1, 16, 16
    gy, x = torch.zeros(n, h, w, 32, device='cuda'), torch.zeros(n, h, w, 32, device='cuda')
    wt = torch.zeros(32, 32, 3, 3, device='cuda')
    gx, gw, gb = torch.empty_like(x), torch.empty_like(wt), torch.empty(32, device='cuda')
    ws = torch.empty(1024, device='cuda')
    assert not L.call_try('dis_conv2d_bwd_fused_f16x2_c16', gy, None, None, 0, None, wt, 32, 32, wt.stride(0), gx, 0, None, None, None, 0,
                          x, None, None, None, 1e-5, gw, gb, ws, n, h, w, 0)


def _net_grads(golden_dir, fused_on):
    """one free-running DIS-MF step of the 64 x 64 fixture; -> (disparity, {parameter: gradient}, entry points called)"""
    import os
    import numpy as np
    from depthinspace_amd import ops, lib
    from tests.test_step_gpu import run_hip_step
    G = np.load(os.path.join(golden_dir, 'mf_64_bs1.npz'))
    old = ops.BWD_FUSED
    ops.BWD_FUSED = fused_on
    lib.profile_start()
    try:
        net, _, _, out = run_hip_step(G)
    finally:
        ops.BWD_FUSED = old
        rec = lib.profile_stop()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}, [r[0] for r in rec]


def test_fusenet_step_with_the_c16_path_on_and_off(golden_dir):
    """every parameter gradient of a small DIS-MF step with the one-launch backward on and off: inside the bar of
    tests/test_step_gpu.py's gradient comparison (2e-3 of the gradient's largest entry), disparity equal"""
    out_on, g_on, names_on = _net_grads(golden_dir, True)
    out_off, g_off, names_off = _net_grads(golden_dir, False)
    assert 'dis_conv2d_bwd_fused_f16x2_c16' in names_on and 'dis_conv2d_bwd_fused_f16x2_c16' not in names_off
    assert torch.equal(out_on, out_off)
    assert g_on.keys() == g_off.keys()
    worst = 0.0
    for k in g_on:
        scale = float(g_off[k].abs().max()) + 1e-20
        err = float((g_on[k] - g_off[k]).abs().max()) / scale
        worst = max(worst, err)
        assert err < 2e-3, (k, err)
    print('worst parameter-gradient difference / largest entry: %.2e' % worst)
