"""GPU: conv_mf's backward in one launch (dis_conv2d_bwd1x1_scaled_gnb, csrc/conv1x1_bwd_fused.hip) against the two launches it
replaces - dis_conv2d_dgrad1x1_scaled_gnb (GroupNorm backward on load, stored operand) and dis_conv2d_wgrad_scaled - and against fp64.
Reference semantics: model/multi_frame_networks.py:406-413 (the 1 x 1 conv over the mask-weighted slots, then GroupNorm) under autograd.

gx must be the two launches' bits.  grad_w / grad_b: within 1e-6 of the largest entry of an fp64 computation on the same operand
(tests/test_bwd_fused_gpu.py's bar) and within twice the two launches' own error.  Shapes: one 4 x 16 tile exactly, ragged by one both
ways, smaller than a tile, several tiles with a ragged last column and row."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, CW = 32, 128
SHAPES = [(4, 16), (5, 17), (3, 7), (9, 40)]


def _inputs(n, h, w, in_act, seed, ranges=False):
    g_ = torch.Generator().manual_seed(seed)
    q = torch.randn(n, h, w, C, generator=g_)
    if in_act:
        q = F.selu(q)
    g = torch.randn(n, h, w, C, generator=g_)
    x = torch.randn(n, h, w, CW, generator=g_)
    if ranges:   # one 1e4 outlier, one sample scaled by 1e-6, one all-zero sample
        g[0, h // 2, w // 2, 5] = 1e4
        g[1] *= 1e-6
        x[1] *= 1e-6
        g[2] = 0
        q[2] = 0
    wt = torch.randn(C, CW, 1, 1, generator=g_) * 0.1
    sc = torch.rand(n, h, w, CW // 32, generator=g_) * 2
    sc = torch.where(torch.rand(n, h, w, CW // 32, generator=g_) < 0.2, torch.zeros_like(sc), sc)
    coef = torch.randn(n * (C + 2) + 4 * n * C + 2, generator=g_) * 0.5
    if ranges:
        coef.view(-1)[2 * (C + 2):3 * (C + 2)] = 0   # the zero sample: gpre = 0
    base = torch.randn(n, h, w, CW, generator=g_)
    return [t.cuda().contiguous() for t in (g, q, x, wt, sc, coef, base)]


def _two_launches(L, ops, g, q, x, wt, sc, coef, base, in_act, accum):
    n, h, w, _ = g.shape
    gpre = torch.full_like(g, float('nan'))
    gx = base.clone()
    L.call('dis_conv2d_dgrad1x1_scaled_gnb', g, q, coef, in_act, gpre, ops._pack_w(wt, CW, 1), gx, sc, n, h, w, C, CW, accum)
    gw, gb = torch.full_like(wt, float('nan')), torch.full((C,), float('nan'), device='cuda')
    ws = torch.empty(L.fn('dis_conv2d_wgrad_workspace')(CW, C, 1, 1), device='cuda')
    L.call('dis_conv2d_wgrad_scaled', x, sc, gpre, gw, gb, ws, n, h, w, CW, CW, C, 1, 1, 0)
    return gpre, gx, gw, gb


def _fused(L, ops, g, q, x, wt, sc, coef, base, in_act, accum):
    n, h, w, _ = g.shape
    gx = base.clone()
    gw, gb = torch.full_like(wt, float('nan')), torch.full((C,), float('nan'), device='cuda')
    wsz = L.fn('dis_conv2d_bwd1x1_scaled_gnb_workspace')(CW, C)
    assert wsz > 0
    ws = torch.empty(wsz, device='cuda')
    assert L.call_try('dis_conv2d_bwd1x1_scaled_gnb', g, q, coef, in_act, ops._pack_w(wt, CW, 1), gx, sc, x, sc, gw, gb, ws, n, h, w,
                      C, CW, accum)
    return gx, gw, gb


def _check(n, h, w, in_act, accum, seed, ranges=False):
    from depthinspace_amd import ops
    L = ops.lib
    t = _inputs(n, h, w, in_act, seed, ranges)
    g, q, x, wt, sc, coef, base = t
    gpre, gx_ref, gw_ref, gb_ref = _two_launches(L, ops, *t, in_act, accum)
    runs = [_fused(L, ops, *t, in_act, accum) for _ in range(3)]
    torch.cuda.synchronize()
    gx, gw, gb = runs[0]
    assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all()
    assert torch.equal(gx, gx_ref), float((gx - gx_ref).abs().max())
    for r in runs[1:]:   # fixed summation order: repeated runs give the same bits
        assert torch.equal(r[0], gx) and torch.equal(r[1], gw) and torch.equal(r[2], gb)
    # fp64 on the operands both paths multiply: x * xscale rounded to fp32 (the kernels' separately rounded multiply), gpre as stored
    xs = (x.view(n, h, w, CW // 32, 32) * sc.unsqueeze(-1)).view(-1, CW).double()
    gp = gpre.view(-1, C).double()
    gw64, gb64 = gp.t() @ xs, gp.sum(0)
    ew, ew_ref = float((gw.view(C, CW).double() - gw64).abs().max()), float((gw_ref.view(C, CW).double() - gw64).abs().max())
    eb, eb_ref = float((gb.double() - gb64).abs().max()), float((gb_ref.double() - gb64).abs().max())
    mw, mb = float(gw64.abs().max()), float(gb64.abs().max())
    print(f'({n},{h},{w}) act {in_act} accum {accum}: grad_w err / max one launch {ew / mw:.3e} two launches {ew_ref / mw:.3e}; '
          f'grad_b {eb / mb:.3e} / {eb_ref / mb:.3e}')
    assert ew <= 1e-6 * mw and eb <= 1e-6 * mb, (ew / mw, eb / mb)
    assert ew <= 2 * ew_ref and eb <= 2 * eb_ref, (ew, ew_ref, eb, eb_ref)


@pytest.mark.parametrize('in_act', [0, 1])
@pytest.mark.parametrize('accum', [0, 1])
@pytest.mark.parametrize('h,w', SHAPES)
def test_one_launch_backward_equals_the_two_launches(h, w, accum, in_act):
    _check(2, h, w, in_act, accum, seed=500 + 7 * h + w + 2 * accum + in_act)


@pytest.mark.parametrize('in_act', [0, 1])
def test_range_case_stays_finite_and_within_the_bars(in_act):
    _check(3, 5, 17, in_act, 0, seed=900 + in_act, ranges=True)


def test_other_shapes_are_unsupported():
    from depthinspace_amd import ops
    L = ops.lib
    assert L.fn('dis_conv2d_bwd1x1_scaled_gnb_workspace')(64, 32) == -1
    assert L.fn('dis_conv2d_bwd1x1_scaled_gnb_workspace')(128, 16) == -1
    t = torch.zeros(4096, device='cuda')
    assert L.call_try('dis_conv2d_bwd1x1_scaled_gnb', t, t, t, 0, t, t, t, t, t, t, t, t, 1, 2, 2, 32, 64, 0) is False
    assert L.call_try('dis_conv2d_bwd1x1_scaled_gnb', t, t, t, 2, t, t, t, t, t, t, t, t, 1, 2, 2, 32, 128, 0) is False


def test_block_backward_agrees_with_the_switch_off(monkeypatch):
    """Block2D3D at (18, 40) with ops.MF_BWD_FUSED on and off: the forward is untouched (outputs within the 1e-5 run-to-run bound), the gradient wrt the block's
    input and every parameter gradient within 1e-6 of its largest entry (tests/test_bench_gpu.py's run-to-run bound)."""
    from depthinspace_amd import ops
    from tests.mf_block_util import block_run
    monkeypatch.setattr(ops, 'MF_BWD_FUSED', False)
    off = block_run(4, 1, 18, 40)
    monkeypatch.setattr(ops, 'MF_BWD_FUSED', True)
    on = block_run(4, 1, 18, 40)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print('on vs off: gradients', max(rel(a, b) for a, b in zip(on[1:], off[1:])))
    assert float((on[0] - off[0]).abs().max()) < 1e-5
    for i, (a, b) in enumerate(zip(on[1:], off[1:])):
        assert rel(a, b) < 1e-6, (i, rel(a, b))
