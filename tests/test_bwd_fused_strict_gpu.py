"""dis_conv2d_bwd_fused_bf16x3 (csrc/conv_bwd_fused_bf16x3.hip): the input gradient and the weight gradient of a 3x3 conv 32 -> 32 in
ONE launch under the strict three-term bf16 split, against the two launches it replaces and against fp64.

Bars: gx BIT-identical to the unfused three-term input-gradient launch (same weight planes, same k-step and product order); grad_w /
grad_b below 1e-6 of the largest fp64 entry and no worse than 2 x the unfused dis_conv2d_wgrad_bf16x3* error + 1e-9."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import conv_split

pytestmark = pytest.mark.gpu

C = 32
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717
FORMS = ['plain', 'plain_accum', 'act', 'act_accum', 'xgn']
SHAPES = [(3, 37, 29), (2, 64, 48), (2, 16, 250), (1, 20, 20), (16, 128, 108)]


def _L():
    from depthinspace_amd import lib
    return lib


def _selu_grad(q):
    return torch.where(q > 0, torch.full_like(q, SELU_SCALE), q + SELU_SCALE * SELU_ALPHA)


def _fp64_wgrad(x, g):
    xn, gn = x.permute(0, 3, 1, 2).double(), g.permute(0, 3, 1, 2).double()
    return torch.nn.grad.conv2d_weight(xn, (C, C, 3, 3), gn, padding=1), gn.sum(dim=(0, 2, 3))


def _gn_eff(x, st, gam, bet, eps):
    n, h, w, c = x.shape
    s = st.view(n, 2)
    mean = (s[:, 0] / (h * w * c)).view(n, 1, 1, 1)
    var = (s[:, 1] / (h * w * c)).view(n, 1, 1, 1) - mean ** 2
    return (x.double() - mean) / torch.sqrt(var + eps) * gam.double() + bet.double()


def _err(a, ref):
    return float((a.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _inputs(form, n, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    q = F.selu(rnd(n, h, w, C))
    gq = rnd(n, h, w, C) * (1.0 + 3.0 * torch.rand(n, 1, 1, 1, generator=gen).cuda())
    wt = (rnd(C, C, 3, 3) * 0.05).contiguous()
    x = rnd(n, h, w, C) * 2.0 + 0.3
    base = rnd(n, h, w, C)
    xg = None
    if form == 'xgn':
        st = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
        xg = (st, (torch.rand(C, generator=gen) + 0.5).cuda(), (torch.randn(C, generator=gen) * 0.1).cuda(), 1e-5)
    return q, gq, wt, x, base, xg


def _unfused(form, gq, q, wt, x, base, xg, n, h, w):
    """the strict mode's two launches: input gradient, weight gradient"""
    from depthinspace_amd import ops
    L = _L()
    accum = form.endswith('accum')
    gx = base.clone()
    if form.startswith('act'):
        L.call('dis_conv2d_dgrad_bf16x3_act', gq, q, ops.ACT_SELU, wt, C, C, wt.stride(0), gx, n, h, w, C, C, 1, 1 if accum else 0)
    else:
        L.call('dis_conv2d_fwd_bf16x3_oihw', gq, wt, 1, C, C, wt.stride(0), None, gx, None, n, h, w, C, C, 3, 1, 1,
               ops.CONV_ACCUM if accum else 0)
    gw, gb = torch.empty(C, C, 3, 3, device='cuda'), torch.empty(C, device='cuda')
    ws = torch.empty(L.fn('dis_conv2d_wgrad_workspace')(C, C, 3, 1), dtype=torch.float32, device='cuda')
    if form == 'xgn':
        L.call('dis_conv2d_wgrad_bf16x3_gn', x, *xg, gq, gw, gb, ws, n, h, w, C, C, C, 3, 1, 1)
    elif form.startswith('act'):
        L.call('dis_conv2d_wgrad_bf16x3_act', x, gq, q, ops.ACT_SELU, gw, gb, ws, n, h, w, C, C, C, 3, 1, 1)
    else:
        L.call('dis_conv2d_wgrad_bf16x3', x, gq, gw, gb, ws, n, h, w, C, C, C, 3, 1, 1)
    return gx, gw, gb


def _fused(form, gq, q, wt, x, base, xg, n, h, w, gw=None, gb=None, gw_rs=0):
    from depthinspace_amd import ops
    L = _L()
    act = form.startswith('act')
    gx = base.clone()
    if gw is None:
        gw = torch.full((C, C, 3, 3), float('nan'), device='cuda')
        gb = torch.full((C,), float('nan'), device='cuda')
    ws = torch.empty(L.fn('dis_conv2d_bwd_fused_bf16x3_workspace')(C), dtype=torch.float32, device='cuda')
    st, gam, bet, eps = xg if xg is not None else (None, None, None, 0.0)
    L.call('dis_conv2d_bwd_fused_bf16x3', gq, q if act else None, ops.ACT_SELU if act else 0, wt, C, C, wt.stride(0), gx,
           1 if form.endswith('accum') else 0, x, st, gam, bet, float(eps), gw, gb, ws, n, h, w, C, gw_rs)
    torch.cuda.synchronize()
    return gx, gw, gb


def _fp64(form, gq, q, x, xg):
    g = gq * _selu_grad(q) if form.startswith('act') else gq   # (the operand as the kernels form it in fp32)
    return _fp64_wgrad(_gn_eff(x, *xg) if form == 'xgn' else x, g)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n,h,w', SHAPES)
def test_bwd_fused_strict_matches_the_two_launches(form, n, h, w):
    with conv_split('bf16x3'):
        q, gq, wt, x, base, xg = _inputs(form, n, h, w, 2000 + 7 * h + w + len(form))
        gx_ref, gw_ref, gb_ref = _unfused(form, gq, q, wt, x, base, xg, n, h, w)
        gx, gw, gb = _fused(form, gq, q, wt, x, base, xg, n, h, w)
        assert torch.equal(gx, gx_ref), float((gx - gx_ref).abs().max())
        gw64, gb64 = _fp64(form, gq, q, x, xg)
        for name, a, r, ref in (('grad_w', gw, gw_ref, gw64), ('grad_b', gb, gb_ref, gb64)):
            e, e_ref = _err(a, ref), _err(r, ref)
            assert e < 1e-6 and e <= 2 * e_ref + 1e-9, (name, e, e_ref)


@pytest.mark.parametrize('form', ['plain', 'act_accum', 'xgn'])
def test_bwd_fused_strict_writes_a_strided_grad_w_slice(form):
    """grad_w as the (c, c, 3, 3) slice [:, c:2c] of a (c, 2c, 3, 3) gradient (conv2d_multi): the slice gets the contiguous result bit for
    bit, the rest of the wider gradient is not touched"""
    n, h, w = 2, 33, 47
    with conv_split('bf16x3'):
        q, gq, wt, x, base, xg = _inputs(form, n, h, w, 77)
        gx0, gw0, gb0 = _fused(form, gq, q, wt, x, base, xg, n, h, w)
        big = torch.full((C, 2 * C, 3, 3), float('nan'), device='cuda')
        gb = torch.full((C,), float('nan'), device='cuda')
        gx1, _, _ = _fused(form, gq, q, wt, x, base, xg, n, h, w, gw=big[:, C:], gb=gb, gw_rs=big.stride(0))
        assert torch.equal(gx1, gx0)
        assert torch.equal(big[:, C:], gw0) and torch.equal(gb, gb0)
        assert bool(torch.isnan(big[:, :C]).all())


def test_bwd_fused_strict_entry_point_refuses_what_it_lacks():
    """DIS_ERR_UNSUPPORTED (call_try -> False) under the two-term split, for 16 channels and for xgn with an activation"""
    from depthinspace_amd import ops
    L = _L()
    n, h, w = 1, 20, 20
    q, gq, wt, x, base, xg = _inputs('xgn', n, h, w, 5)
    ws = torch.empty(L.fn('dis_conv2d_bwd_fused_bf16x3_workspace')(C), dtype=torch.float32, device='cuda')
    gw, gb, gx = torch.empty(C, C, 3, 3, device='cuda'), torch.empty(C, device='cuda'), base.clone()
    args = lambda act, st, c: (gq, q, act, wt, C, C, wt.stride(0), gx, 0, x, st, xg[1], xg[2], 1e-5, gw, gb, ws, n, h, w, c, 0)
    with conv_split('f16x2'):
        assert not L.call_try('dis_conv2d_bwd_fused_bf16x3', *args(0, None, C))
    with conv_split('bf16x3'):
        assert not L.call_try('dis_conv2d_bwd_fused_bf16x3', *args(0, None, 16))
        assert not L.call_try('dis_conv2d_bwd_fused_bf16x3', *args(ops.ACT_SELU, xg[0], C))
    assert L.fn('dis_conv2d_bwd_fused_bf16x3_workspace')(16) < 0


def _hard(case, gen):
    if case == 'exponent_ramp':
        n, h, w = 4, 256, 256
        x, g = torch.randn(n, h, w, C, generator=gen), torch.randn(n, h, w, C, generator=gen)
        r = torch.randint(0, 4, (n, h // 16, w // 16), generator=gen)
        sc = torch.pow(2.0, 7.0 * r.double()).float().repeat_interleave(16, 1).repeat_interleave(16, 2).unsqueeze(-1)
        return x * sc, g * sc
    n, h, w = 3, 37, 45
    x, g = torch.randn(n, h, w, C, generator=gen), torch.randn(n, h, w, C, generator=gen)
    if case == 'tiny_sample':
        x[1] *= 1e-6
        g[1] *= 1e-6
    else:   # outlier_pixel: one 1e4 pixel in x and one in g, in different samples
        x[0, 20, 11] = 1e4
        g[1, 7, 40] = 1e4
    return x, g


@pytest.mark.parametrize('case', ['tiny_sample', 'outlier_pixel', 'exponent_ramp'])
@pytest.mark.parametrize('form', ['plain', 'act', 'act_accum', 'xgn'])
def test_bwd_fused_strict_is_reproducible_on_hard_inputs(case, form):
    gen = torch.Generator().manual_seed(31 + len(case))
    x, g = (t.cuda() for t in _hard(case, gen))
    n, h, w, _ = x.shape
    q = F.selu(torch.randn(n, h, w, C, generator=gen)).cuda()
    wt = (torch.randn(C, C, 3, 3, generator=gen) * 0.05).cuda()
    base = torch.randn(n, h, w, C, generator=gen).cuda() if form.endswith('accum') else torch.zeros_like(x)
    xg = None
    if form == 'xgn':
        st = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
        xg = (st, (torch.rand(C, generator=gen) + 0.5).cuda(), (torch.randn(C, generator=gen) * 0.1).cuda(), 1e-5)
    with conv_split('bf16x3'):
        a = _fused(form, g, q, wt, x, base, xg, n, h, w)
        b = _fused(form, g, q, wt, x, base, xg, n, h, w)
        ref = _unfused(form, g, q, wt, x, base, xg, n, h, w)
    for u, v in zip(a, b):
        assert bool(torch.isfinite(u).all())
        assert torch.equal(u, v)
    assert torch.equal(a[0], ref[0])
    gw64, gb64 = _fp64(form, g, q, x, xg)
    for name, u, r, ref64 in (('grad_w', a[1], ref[1], gw64), ('grad_b', a[2], ref[2], gb64)):
        e, e_ref = _err(u, ref64), _err(r, ref64)
        assert e < 1e-6 and e <= 2 * e_ref + 1e-9, (name, e, e_ref)


def _run_ops(fn, params, inputs):
    """forward + backward of fn under the strict split: (output, input grads, param grads, names of the entry points the step called)"""
    from depthinspace_amd import lib
    for t in list(params) + list(inputs):
        t.grad = None
    lib.profile_start()
    out = fn()
    (out * out).sum().backward()
    names = [r[0] for r in lib.profile_stop()]
    return out.detach(), [t.grad.clone() for t in inputs], [p.grad.clone() for p in params], names


def _ops_case(kind):
    """-> (forward, params, inputs, fp64 reference of the param grads from (output, params, inputs))"""
    from depthinspace_amd import ops
    from depthinspace_amd.model import multi_frame_networks as M
    torch.manual_seed(3)
    n, h, w = 2, 40, 36
    if kind == 'resnet_block':
        blk = M.ResNetBlock(C).cuda()
        x = torch.randn(n, h, w, C, device='cuda').requires_grad_(True)

        def ref64(out, params, inputs):   # the block's chain in fp64 (model/multi_frame_networks.py ResNetBlock)
            p = [t.detach().double().requires_grad_(True) for t in params]
            pd = dict(zip([k for k, _ in blk.named_parameters()], p))
            xd = inputs[0].detach().double().permute(0, 3, 1, 2)
            o = F.selu(F.conv2d(xd, pd['conv1.weight'], pd['conv1.bias'], padding=1))
            o = F.group_norm(o, 1, pd['bn1.weight'], pd['bn1.bias'], eps=1e-5)
            o = F.group_norm(F.conv2d(o, pd['conv2.weight'], pd['conv2.bias'], padding=1), 1, pd['bn2.weight'], pd['bn2.bias'], eps=1e-5)
            o = F.selu(o + xd)
            (o * o).sum().backward()
            return [t.grad for t in p]
        return (lambda: blk(x)), list(blk.parameters()), [x], ref64
    a = torch.randn(n, h, w, C, device='cuda').requires_grad_(True)
    b = torch.randn(n, h, w, C, device='cuda').requires_grad_(True)
    wt = (torch.randn(C, 2 * C, 3, 3, device='cuda') * 0.05).requires_grad_(True)
    bias = (torch.randn(C, device='cuda') * 0.1).requires_grad_(True)

    def ref64(out, params, inputs):   # the weight-gradient operand as the kernels form it in fp32 (2 y SELU'(y)), convolved in fp64
        gpre = (2.0 * out) * _selu_grad(out)
        xc = torch.cat([t.detach() for t in inputs], dim=3).permute(0, 3, 1, 2).double()
        gn = gpre.permute(0, 3, 1, 2).double()
        return [torch.nn.grad.conv2d_weight(xc, tuple(wt.shape), gn, padding=1), gn.sum(dim=(0, 2, 3))]
    return (lambda: ops.conv2d_multi((a, b), wt, bias, 1, ops.ACT_SELU)[0]), [wt, bias], [a, b], ref64


@pytest.mark.parametrize('kind', ['resnet_block', 'conv2d_multi'])
def test_strict_backward_through_ops_takes_the_fused_launch(kind, monkeypatch):
    """every form selected (the step's default selects none: all measured slower fused): the backward runs the
    one launch; gx bit for bit as the two launches, parameter gradients vs fp64 no worse than 2 x the two launches' error + 1e-9,
    and, where the fp64 reference is the conv alone (conv2d_multi's two weight slices and bias), below 1e-6 of its largest entry"""
    from depthinspace_amd import ops
    with conv_split('bf16x3'):
        fn, params, inputs, ref64 = _ops_case(kind)
        monkeypatch.setattr(ops, 'BWD_FUSED_STRICT', frozenset(ops.BWD_FUSED_STRICT_FORMS))
        out_f, gi_f, gp_f, names = _run_ops(fn, params, inputs)
        assert 'dis_conv2d_bwd_fused_bf16x3' in names, sorted(set(names))
        monkeypatch.setattr(ops, 'BWD_FUSED', False)
        out_u, gi_u, gp_u, names_u = _run_ops(fn, params, inputs)
        assert 'dis_conv2d_bwd_fused_bf16x3' not in names_u
    assert torch.equal(out_f, out_u)
    for a, b in zip(gi_f, gi_u):
        assert torch.equal(a, b), float((a - b).abs().max())
    refs = ref64(out_u, params, inputs)
    for i, (a, b, r) in enumerate(zip(gp_f, gp_u, refs)):
        e, e_ref = _err(a, r), _err(b, r)
        assert e <= 2 * e_ref + 1e-9, (i, e, e_ref)
        if kind == 'conv2d_multi':
            assert e < 1e-6, (i, e)


@pytest.mark.parametrize('name', ['mf_64_bs1', 'mf_128_bs1'])
def test_strict_mf_step_matches_reference(golden_dir, name, monkeypatch):
    """the free-running DIS-MF step under the strict split with every form on the one launch, at the bars of tests/test_step_gpu.py"""
    from depthinspace_amd import ops
    from tests import test_step_gpu
    monkeypatch.setattr(ops, 'BWD_FUSED_STRICT', frozenset(ops.BWD_FUSED_STRICT_FORMS))
    with conv_split('bf16x3'):
        test_step_gpu.test_mf_step_matches_reference(golden_dir, name)


def test_strict_graphed_step_matches_eager(monkeypatch):
    """trainer.GraphedStep under the strict split, every form on the one launch: two replays of the captured step land on the
    parameters of two eager steps"""
    from depthinspace_amd import ops, synth
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam, GraphedStep
    from tests.test_track_length_gpu import _args
    H = W = 64
    monkeypatch.setattr(ops, 'BWD_FUSED_STRICT', frozenset(ops.BWD_FUSED_STRICT_FORMS))
    with conv_split('bf16x3'):
        settings = synth.make_settings(H, W)
        torch.manual_seed(0)
        wk = multi_frame_worker.Worker(_args(1, 4), settings=settings)
        net = multi_frame_networks.FuseNet((H, W), settings.K, settings.baseline, track_length=4).cuda()
        wk.build_losses()
        wk.current_epoch = 2
        opt = FlatAdam(net.parameters(), lr=1e-4)
        batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(settings, 1, 4, seed=77).items()}
        state = (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.state_dev)
        snap = [t.clone() for t in state]
        eager = GraphedStep(wk, net, opt, batch, use_graph=False)
        for _ in range(2):
            eager.run()
        torch.cuda.synchronize()
        p_eager, l_eager = opt.flat_p.clone(), eager.losses()
        graphed = GraphedStep(wk, net, opt, batch, use_graph=True, warmup=1, strict=True)
        graphed.run()
        torch.cuda.synchronize()
        assert graphed.mode == 'graph'
        for t, c in zip(state, snap):
            t.copy_(c)
        for _ in range(2):
            graphed.run()
        torch.cuda.synchronize()
    assert float((opt.flat_p - p_eager).abs().max()) < 2.5e-4
    assert float((opt.flat_p - p_eager).abs().mean()) < 2e-6
    np.testing.assert_allclose(graphed.losses(), l_eager, rtol=2e-3, atol=1e-5)
