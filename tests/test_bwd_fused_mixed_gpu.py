"""dis_conv2d_bwd_fused_f16x2_c16 at the mixed pairs (csrc/conv_bwd_fused_mixed.hip): the input gradient and the weight gradient of a
3x3 conv 16 -> 32 or 32 -> 16 in ONE launch, against the two launches it replaces and against fp64.

Reference semantics: torch.nn.Conv2d's backward of conv3, ref_conv and final_conv (model/multi_frame_networks.py:146-150,230-251).
Bars (tests/test_bwd_fused_c16_gpu.py's): gx BIT-identical to the unfused input-gradient launch, the GroupNorm-backward channel sums
within 1e-6, grad_w / grad_b within 1e-6 of the largest entry of the fp64 result and no further from fp64 than twice the error of the
two launches replaced."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# plain_act: operand gy SELU'(y), gx written (conv3).  act_sums_res: the same operand, gx = conv_T(.) SELU'(x) written, plus the
# channel sums of gx and gx x2 (final_conv, ref_conv's 16-channel source: dis_conv2d_dgrad_bf16x3_act_gnsums_res's arithmetic)
CASES = [('plain_act', 16, 32), ('plain_act', 32, 16), ('act_sums_res', 16, 32), ('act_sums_res', 32, 16)]
# ragged both ways, one tile high, smaller than the grid, one pixel past a tile both ways; and 630 tiles of 16 x 16 over three samples:
# more tiles than workgroups, so a workgroup walks several tiles, prefetches across them and flushes its channel sums at a sample change
SHAPES = [(3, 37, 29), (2, 16, 50), (1, 20, 20), (2, 33, 17), (3, 224, 240)]
SELU_S, SELU_A = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def _selu_grad(q):
    return torch.where(q > 0, torch.full_like(q, SELU_S), q + SELU_S * SELU_A)


def _fp64_wgrad(x, gpre):
    xn = x.permute(0, 3, 1, 2).double()
    gn = gpre.permute(0, 3, 1, 2).double()
    gw = torch.nn.grad.conv2d_weight(xn, (gn.shape[1], xn.shape[1], 3, 3), gn, padding=1)
    return gw, gn.sum(dim=(0, 2, 3))


def _fused(L, form, gy, y, wt, x, x2, gw, gb, stride=0, in_act=None):
    """-> (ok, gx, channel sums (n, 2, cin) | None)"""
    from depthinspace_amd import ops
    cout, cin = wt.shape[0], wt.shape[1]
    n, h, w, _ = x.shape
    sums = form == 'act_sums_res'
    slots = L.fn('dis_conv2d_bwd_fused_c16_slots')(cin, cout)
    ws = torch.empty(L.fn('dis_conv2d_bwd_fused_c16_workspace')(cin, cout), dtype=torch.float32, device='cuda')
    gx = torch.full_like(x, float('nan'))
    ab = torch.zeros(n * slots * 2 * cin, dtype=torch.float64, device='cuda') if sums else None
    in_act = ops.ACT_SELU if in_act is None else in_act
    ok = L.call_try('dis_conv2d_bwd_fused_f16x2_c16', gy, y if in_act else None, None, in_act, None, wt, cout, cin, wt.stride(0), gx, 0,
                    x2 if sums else None, x if sums else None, ab, slots, x, None, None, None, 1e-5, gw, gb, ws, n, h, w, stride)
    torch.cuda.synchronize()
    return ok, gx, (ab.view(n, slots, 2, cin).sum(dim=1) if sums else None)


def _two_launches(L, form, gy, y, wt, x, x2):
    """-> (gx, channel sums | None, grad_w, grad_b) of the launches the fused one replaces"""
    from depthinspace_amd import ops
    cout, cin = wt.shape[0], wt.shape[1]
    n, h, w, _ = x.shape
    gx = torch.full_like(x, float('nan'))
    ab = None
    if form == 'act_sums_res':
        slots = L.fn('dis_conv2d_gnsums_slots')()
        ab = torch.zeros(n * slots * 2 * cin, dtype=torch.float64, device='cuda')
        L.call('dis_conv2d_dgrad_bf16x3_act_gnsums_res', gy, y, wt, cout, cin, wt.stride(0), gx, x, x2, ab, n, h, w, cout, cin, 1)
        ab = ab.view(n, slots, 2, cin).sum(dim=1)
    else:
        L.call('dis_conv2d_dgrad_bf16x3_act', gy, y, ops.ACT_SELU, wt, cout, cin, wt.stride(0), gx, n, h, w, cout, cin, 1, 0)
    gw, gb = torch.empty(cout, cin, 3, 3, device='cuda'), torch.empty(cout, device='cuda')
    ws = torch.empty(L.fn('dis_conv2d_wgrad_workspace')(cin, cout, 3, 1), dtype=torch.float32, device='cuda')
    L.call('dis_conv2d_wgrad_bf16x3_act', x, gy, y, ops.ACT_SELU, gw, gb, ws, n, h, w, cin, cin, cout, 3, 1, 1)
    torch.cuda.synchronize()
    return gx, ab, gw, gb


def _check(tag, fused, ref, x, gy, y):
    gx, ab, gw, gb = fused
    gx_ref, ab_ref, gw_ref, gb_ref = ref
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    assert torch.equal(gx, gx_ref), float((gx - gx_ref).abs().max())
    if ab_ref is not None:
        assert float((ab - ab_ref).abs().max()) <= 1e-6 * float(ab_ref.abs().max()), float((ab - ab_ref).abs().max())
    gw64, gb64 = _fp64_wgrad(x, gy * _selu_grad(y))
    sw, sb = float(gw64.abs().max()), float(gb64.abs().max())
    e_new, e_old = float((gw.double() - gw64).abs().max()) / sw, float((gw_ref.double() - gw64).abs().max()) / sw
    b_new, b_old = float((gb.double() - gb64).abs().max()) / sb, float((gb_ref.double() - gb64).abs().max()) / sb
    print(tag, 'grad_w err / largest: fused %.2e, two launches %.2e; grad_b %.2e / %.2e' % (e_new, e_old, b_new, b_old))
    assert e_new < 1e-6, (e_new, e_old)
    assert b_new < 1e-6, (b_new, b_old)
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert b_new <= 2 * b_old, (b_new, b_old)


@pytest.mark.parametrize('n,h,w', SHAPES)
@pytest.mark.parametrize('form,cin,cout', CASES)
def test_bwd_fused_mixed_matches_the_two_launches(form, cin, cout, n, h, w):
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_get_conv_split')() == 1
    g_ = torch.Generator().manual_seed(3000 + 7 * h + w + len(form) + cin)
    rnd = lambda *s: torch.randn(*s, generator=g_).cuda()
    y = F.selu(rnd(n, h, w, cout))
    gy = rnd(n, h, w, cout) * (1.0 + 3.0 * torch.rand(n, 1, 1, 1, generator=g_).cuda())   # per-sample magnitudes differ: the running scales move
    wt = (rnd(cout, cin, 3, 3) * 0.05).contiguous()
    x = F.selu(rnd(n, h, w, cin) * 2.0 + 0.3)   # (an activation output: the result is multiplied with SELU'(x) in act_sums_res)
    x2 = rnd(n, h, w, cin)
    ref = _two_launches(L, form, gy, y, wt, x, x2)
    gw, gb = torch.full((cout, cin, 3, 3), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda')
    ok, gx, ab = _fused(L, form, gy, y, wt, x, x2, gw, gb)
    assert ok, 'no instance for a form the step uses'
    _check((form, (cin, cout), (n, h, w)), (gx, ab, gw, gb), ref, x, gy, y)


@pytest.mark.parametrize('form,cin,cout', CASES)
def test_bwd_fused_mixed_is_reproducible_and_handles_extreme_ranges(form, cin, cout):
    """a 1e4 outlier in one sample, a 1e-6 sample, zeros in another: the running dW exponent moves, nothing overflows, and the launch
    repeats bit for bit (fixed summation orders, no atomics)"""
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_get_conv_split')() == 1
    n, h, w = 5, 48, 40
    g_ = torch.Generator().manual_seed(77)
    gy = torch.randn(n, h, w, cout, generator=g_).cuda()
    y = F.selu(torch.randn(n, h, w, cout, generator=g_)).cuda()
    x = F.selu(torch.randn(n, h, w, cin, generator=g_)).cuda()
    x2 = torch.randn(n, h, w, cin, generator=g_).cuda()
    gy[1] *= 1e-6
    x[2] = 0.0
    gy[3, 7, 9, 5] = 1e4
    y[3, 7, 9, 5] = 1.0
    x[4, 30, 2, 11] = 3e3
    gy[0, :16, :16] = 0.0
    wt = (torch.randn(cout, cin, 3, 3, generator=g_) * 0.05).cuda()
    outs = []
    for rep in range(3):
        gw, gb = torch.empty(cout, cin, 3, 3, device='cuda'), torch.empty(cout, device='cuda')
        ok, gx, ab = _fused(L, form, gy, y, wt, x, x2, gw, gb)
        assert ok
        outs.append((gx, gw, gb) + ((ab,) if ab is not None else ()))
    for o in outs[1:]:
        assert all(torch.equal(a_, b_) for a_, b_ in zip(o, outs[0]))
    ref = _two_launches(L, form, gy, y, wt, x, x2)
    _check(('range case', form, (cin, cout)), (outs[0][0], outs[0][3] if form == 'act_sums_res' else None, outs[0][1], outs[0][2]), ref,
           x, gy, y)


def test_bwd_fused_mixed_writes_a_slice_of_a_wider_weight_gradient():
    """grad_w_row_stride: ref_conv's 16-channel source writes columns 32 .. 47 of the (32, 48, 3, 3) gradient in place: the slice
    equals the contiguous result bit for bit, every other column is untouched."""
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_get_conv_split')() == 1
    cin, cout, n, h, w = 16, 32, 2, 40, 56
    g_ = torch.Generator().manual_seed(5)
    gy = torch.randn(n, h, w, cout, generator=g_).cuda()
    y = F.selu(torch.randn(n, h, w, cout, generator=g_)).cuda()
    x = F.selu(torch.randn(n, h, w, cin, generator=g_)).cuda()
    x2 = torch.randn(n, h, w, cin, generator=g_).cuda()
    wide_w = (torch.randn(cout, 48, 3, 3, generator=g_) * 0.05).cuda()
    wt = wide_w[:, 32:48]   # (the weight itself is such a slice in the step: w_row_stride)
    ref = torch.empty(cout, cin, 3, 3, device='cuda')
    gb0 = torch.empty(cout, device='cuda')
    ok, gx0, ab0 = _fused(L, 'act_sums_res', gy, y, wt, x, x2, ref, gb0)
    assert ok
    wide = torch.full((cout, 48, 3, 3), 7.0, device='cuda')
    sl = wide[:, 32:48]
    gb1 = torch.empty(cout, device='cuda')
    ok, gx1, ab1 = _fused(L, 'act_sums_res', gy, y, wt, x, x2, sl, gb1, stride=sl.stride(0))
    assert ok and torch.equal(gx0, gx1) and torch.equal(gb0, gb1) and torch.equal(ab0, ab1)
    assert torch.equal(sl, ref)
    assert bool((wide[:, :32] == 7.0).all())
    # and against the two launches, whose weight is the same slice
    gx_ref = _two_launches(L, 'act_sums_res', gy, y, wt, x, x2)[0]
    assert torch.equal(gx0, gx_ref)


def test_bwd_fused_mixed_entry_point_answers_for_its_pairs_only():
    from depthinspace_amd import ops
    L = ops.lib
    wsf, slf = L.fn('dis_conv2d_bwd_fused_c16_workspace'), L.fn('dis_conv2d_bwd_fused_c16_slots')
    assert wsf(16, 32) >= 0 and wsf(32, 16) >= 0 and slf(16, 32) > 0 and slf(32, 16) > 0
    assert wsf(32, 32) < 0 and wsf(8, 16) < 0
    # a form without an instance (the plain operand gy): "unsupported", and nothing is launched - no output is written
    cin, cout, n, h, w = 16, 32, 1, 16, 16
    gy, y = torch.ones(n, h, w, cout, device='cuda'), torch.ones(n, h, w, cout, device='cuda')
    x = torch.ones(n, h, w, cin, device='cuda')
    wt = torch.ones(cout, cin, 3, 3, device='cuda')
    gw, gb = torch.full((cout, cin, 3, 3), 7.0, device='cuda'), torch.full((cout,), 7.0, device='cuda')
    ok, gx, _ = _fused(L, 'plain', gy, y, wt, x, None, gw, gb, in_act=0)
    assert not ok
    assert bool(torch.isnan(gx).all()) and bool((gw == 7.0).all()) and bool((gb == 7.0).all())


def _net_step(golden_dir, fused_on):
    """one free-running DIS-MF step of the 64 x 64 fixture; -> (disparity, {parameter: gradient}, [(entry point, int args)])"""
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
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}, [(r[0], tuple(r[1])) for r in rec]


def test_fusenet_step_runs_the_mixed_layers_in_one_launch(golden_dir):
    """final_conv (32 -> 16), ref_conv's 16-channel source and conv3 (16 -> 32) go through the one-launch entry point and leave no
    activation weight-gradient launch behind; with the path on and off the disparity is equal and every parameter gradient is inside
    the bar of tests/test_step_gpu.py's gradient comparison (2e-3 of the gradient's largest entry)"""
    out_on, g_on, rec_on = _net_step(golden_dir, True)
    out_off, g_off, rec_off = _net_step(golden_dir, False)
    # int args of the entry point: in_act, w_o, w_i, ...; of dis_conv2d_wgrad_bf16x3_act: act, n, h, w, cin_pad, cin, cout, ...
    fused_pairs = [a[1:3] for nm, a in rec_on if nm == 'dis_conv2d_bwd_fused_f16x2_c16']
    print('one-launch calls (w_o, w_i):', sorted(set(fused_pairs)), len(fused_pairs))
    assert fused_pairs.count((16, 32)) >= 1, 'final_conv'
    assert fused_pairs.count((32, 16)) >= 2, "ref_conv's 16-channel source and conv3"
    wg_on = [a[5:7] for nm, a in rec_on if nm == 'dis_conv2d_wgrad_bf16x3_act']
    wg_off = [a[5:7] for nm, a in rec_off if nm == 'dis_conv2d_wgrad_bf16x3_act']
    assert (32, 16) in wg_off and (16, 32) in wg_off, wg_off
    assert (32, 16) not in wg_on and (16, 32) not in wg_on, wg_on
    assert not any(nm == 'dis_conv2d_bwd_fused_f16x2_c16' for nm, _ in rec_off)
    assert torch.equal(out_on, out_off)
    assert g_on.keys() == g_off.keys()
    worst = 0.0
    for k in g_on:
        scale = float(g_off[k].abs().max()) + 1e-20
        err = float((g_on[k] - g_off[k]).abs().max()) / scale
        worst = max(worst, err)
        assert err < 2e-3, (k, err)
    print('worst parameter-gradient difference / largest entry: %.2e' % worst)
