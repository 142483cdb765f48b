"""GPU: the order-free backward of the flow-consistency loss (dis_geo_loss_bwd_det / _bwd_multi_det, ops.set_geo_bwd_det, DIS_GEO_BWD=det,
Worker(geo_bwd='det')).

Pass 1 adds -sigma rint(w 2^32) per valid bilinear tap to a 64-bit integer cell per term and pixel (sigma = mask x sign) and stores
the depth0 addend; pass 2 sums the terms of every gradient plane in table order in double, rounds to fp32 once and adds to the plane.
Integer sums do not depend on the order of arrival, so the same inputs give the same bits on every call - which the atomic form
(float atomics, terms sharing a frame running concurrently) does not promise.

  * fp64 parity with the bars, shapes and leave-out cap of tests/test_pixel_ops_fp64_gpu.py::test_geo_loss_dir / _all_vs_fp64
  * eight launches on the same inputs are torch.equal, up to 4096 addends per cell
  * g_depth1 equals a numpy restatement (fp32 taps and weights as bilin_zeros spells them, int64 sums) bit for bit: the
    order-free semantics, not one lucky order
  * det against atomic within the golden tolerance at every pixel; the single-term g_depth0 bit for bit
  * empty mask, GradAccum, 17 terms, the workspace query
  * a 64 x 64 training step: the geometric terms' gradient wrt the disparities repeats bit for bit; captured == eager
"""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import pixel_ref as P
from tests import test_pixel_ops_fp64_gpu as T   # _geo_term, cap: the construction of the atomic form's fp64 tests

pytestmark = pytest.mark.gpu

f32 = np.float32
TWO32 = f32(4294967296.0)


@pytest.fixture(autouse=True)
def det_mode():
    from depthinspace_amd import ops
    prev = ops.set_geo_bwd_det(True)
    yield
    ops.set_geo_bwd_det(prev)


@functools.lru_cache(maxsize=None)
def _input(bs, h, w, tl=2, empty=False):
    return P.geo_input(bs, h, w, tl=tl, empty=empty)


@functools.lru_cache(maxsize=None)
def _det_term(bs, h, w, i, j, mode, gscale=0.7, tl=2, empty=False):
    """T._geo_term in det mode, once per case: (kernel, fp64 reference, fp32 oracle, mask, keeps)"""
    from depthinspace_amd import ops, lib
    from tests import bitexact as B
    assert ops.GEO_BWD_DET
    return T._geo_term(ops, lib, B, _input(bs, h, w, tl, empty), i, j, mode, gscale)


# ---------------------------------------------------------------------------------------------------------------- 1. single term
@pytest.mark.parametrize('mode', ['mf', 'sf'])
@pytest.mark.parametrize('bs_h_w', P.GEO_SHAPES)
def test_det_dir_vs_fp64(bs_h_w, mode):
    """the cases, bars and leave-out cap of test_geo_loss_dir"""
    bs, h, w = bs_h_w
    for (i, j) in ((0, 1), (1, 0)):
        ker, ref, ora, m, (k0, k1, active) = _det_term(bs, h, w, i, j, mode)
        assert 0.0 < float(m.mean()) < 1.0
        T.cap(k0, f'geo det {bs_h_w} {mode} depth0')
        T.cap(k1, f'geo det {bs_h_w} {mode} depth1')
        tag = f'det {mode} {bs}x{h}x{w} {i}->{j}'
        for k, keep, name in ((1, k0, 'g_depth0'), (2, k1, 'g_depth1')):
            scale = float(ref[k].abs().max())
            assert scale > 0
            P.check('geo_loss', f'{name} ' + tag, ker[k], ora[k], ref[k], 2e-5 * scale, 1e-4, keep)


# ---------------------------------------------------------------------------------------------------------------- 2. multi term
def _pairs(mode):
    return [(i, j) for i in range(3) for j in range(3) if i != j] if mode == 'mf' else [(0, 1), (1, 2), (2, 0)]


def _all_grad(g, mode, pairs, gvec):
    """depth gradient (tl, bs, 1, h, w) of sum_k gvec[k] term_k through ops.geo_loss_all, on the device"""
    from depthinspace_amd import ops, lib
    K, Ki = lib.host_floats(g['K'].reshape(-1)), lib.host_floats(g['Kinv'].reshape(-1))
    depth = g['depth'].cuda().requires_grad_(True)
    flows = [(g['flow'][(i, j)].cuda(), g['flow'][(j, i)].cuda()) for (i, j) in pairs]
    vals = ops.geo_loss_all(depth, g['amb'].cuda(), g['pdepth'].cuda() if mode == 'mf' else None, g['R'].cuda(), g['t'].cuda(), K, Ki,
                            P.GEO_CLAMP if mode == 'sf' else -1.0, pairs, flows)
    (vals * gvec.cuda()).sum().backward()
    return depth.grad


@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_det_all_vs_fp64(mode):
    """the construction of test_geo_loss_all_vs_fp64: three frames, every frame depth0 of some terms and depth1 of others, unequal
    gscale per term"""
    bs, h, w = 3, 33, 41
    g = _input(bs, h, w, 3)
    pairs = _pairs(mode)
    gvec = torch.linspace(0.5, 1.5, len(pairs))
    ref_g, ora_g = torch.zeros(3, bs, 1, h, w, dtype=P.F64), torch.zeros(3, bs, 1, h, w)
    keep = torch.ones(3, bs, 1, h, w, dtype=torch.bool)
    for k, (i, j) in enumerate(pairs):
        _, ref, ora, m, (k0, k1, _) = _det_term(bs, h, w, i, j, mode, float(gvec[k]), 3)
        ref_g[i] += ref[1]; ref_g[j] += ref[2]
        ora_g[i] += ora[1]; ora_g[j] += ora[2]
        keep[i] &= k0; keep[j] &= k1
    T.cap(keep, f'geo det all {mode}')
    grad = _all_grad(g, mode, pairs, gvec)
    scale = float(ref_g.abs().max())
    P.check('geo_loss', f'det all-terms grad {mode}', grad.cpu(), ora_g, ref_g, 2e-5 * scale, 1e-4, keep)


# ---------------------------------------------------------------------------------------------------------------- 3. repeats
def _dir_grads(g, i, j, mode, gscale=0.7):
    from depthinspace_amd import ops, lib
    K, Ki = lib.host_floats(g['K'].reshape(-1)), lib.host_floats(g['Kinv'].reshape(-1))
    d0, d1 = g['depth'][i].cuda().requires_grad_(True), g['depth'][j].cuda().requires_grad_(True)
    val, _ = ops.geo_loss_dir(d0, d1, g['flow'][(i, j)].cuda(), g['flow'][(j, i)].cuda(), g['amb'][i].cuda(), g['amb'][j].cuda(),
                              g['pdepth'][j].cuda() if mode == 'mf' else None, g['R'][i].cuda(), g['t'][i].cuda(), g['R'][j].cuda(),
                              g['t'][j].cuda(), K, Ki, P.GEO_CLAMP if mode == 'sf' else -1.0)
    (val * gscale).backward()
    return d0.grad, d1.grad


REPEATS = 8


@pytest.mark.parametrize('case', ['multi 3x33x41', 'multi 1x130x94', 'single 2x512x432'])
def test_det_repeats_bit_for_bit(case):
    runs = []
    for _ in range(REPEATS):
        if case == 'multi 3x33x41':
            pairs = _pairs('mf')
            runs.append(_all_grad(_input(3, 33, 41, 3), 'mf', pairs, torch.linspace(0.5, 1.5, len(pairs))))
        elif case == 'multi 1x130x94':
            runs.append(_all_grad(_input(1, 130, 94), 'sf', [(0, 1), (1, 0)], torch.tensor([0.6, 1.3])))
        else:
            runs.append(torch.stack(_dir_grads(_input(2, 512, 432), 0, 1, 'mf')))
    assert float(runs[0].abs().max()) > 0
    for r in runs[1:]:
        assert torch.equal(r, runs[0]), f'{case}: {int((r != runs[0]).sum())} elements differ between two launches'


def _convergent_input():
    """1 x 64 x 64: every source pixel's flow points at (20.37, 31.61) - 4096 addends in each of four cells of depth1;
    depth1 = depth0 + 0.5, so d1 - depth10 is about -0.5 everywhere (no pixel near the kink of |.|); all-ones mask"""
    g = _input(1, 64, 64)
    yy, xx = np.meshgrid(np.arange(64, dtype=np.float64), np.arange(64, dtype=np.float64), indexing='ij')
    flow = torch.from_numpy(np.stack([20.37 - xx, 31.61 - yy])[None].astype(np.float32))
    depth0 = g['depth'][0]
    return dict(depth0=depth0, depth1=depth0 + 0.5, flow=flow, R0=g['R'][0], t0=g['t'][0], R1=g['R'][1], t1=g['t'][1], K=g['K'],
                Kinv=g['Kinv'], mask=torch.ones_like(depth0))


def _call_det(c, gscale, single=True):
    """dis_geo_loss_bwd_det through lib.call with a hand-made mask and mask sum -> (g_depth0, g_depth1)"""
    from depthinspace_amd import lib
    bs, _, h, w = c['depth0'].shape
    dev = {k: c[k].cuda().contiguous() for k in ('depth0', 'depth1', 'flow', 'R0', 't0', 'R1', 't1', 'mask')}
    K, Ki = lib.host_floats(c['K'].reshape(-1)), lib.host_floats(c['Kinv'].reshape(-1))
    acc = torch.zeros(lib.fn('dis_geo_loss_acc_doubles')(), dtype=torch.float64).cuda()
    acc[1] = float(c['mask'].double().sum())
    gs = torch.tensor([gscale], dtype=torch.float32).cuda()
    g0, g1 = torch.zeros_like(dev['depth0']), torch.zeros_like(dev['depth1'])
    ws = torch.empty(lib.fn('dis_geo_loss_bwd_det_workspace')(1, bs, h, w), dtype=torch.uint8).cuda()
    lib.call('dis_geo_loss_bwd_det', dev['depth0'], dev['depth1'], dev['flow'], dev['R0'], dev['t0'], dev['R1'], dev['t1'], K, Ki, -1.0,
             dev['mask'], acc, gs, g0, g1, bs, h, w, ws)
    return g0, g1


def test_det_convergent_flows():
    """4096 addends per destination cell: bit for bit across eight launches, equal to the host restatement, and within the
    single-term bars of the fp64 gradients with the same mask"""
    c = _convergent_input()
    args = (c['depth0'], c['depth1'], c['flow'], c['R0'], c['t0'], c['R1'], c['t1'], c['K'], c['Kinv'], c['mask'])
    k0, k1, _ = P.geo_keep(*args, None)
    T.cap(k0, 'convergent depth0')
    T.cap(k1, 'convergent depth1')
    runs = [torch.stack(_call_det(c, 0.7)) for _ in range(REPEATS)]
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    g0, g1 = runs[0][0].cpu(), runs[0][1].cpu()
    assert int((g1 != 0).sum()) == 4
    _, r0, r1 = P.geo_dir_grads(*args, None, 0.7)
    # (no fp32 oracle takes a hand-made mask: the reference stands in for it, which leaves the golden tolerance alone as the bar)
    for name, ker, ref, keep in (('g_depth0', g0, r0, k0), ('g_depth1', g1, r1, k1)):
        scale = float(ref.abs().max())
        assert scale > 0
        P.check('geo_loss', f'{name} det convergent 1x64x64', ker, ref, ref, 2e-5 * scale, 1e-4, keep)
    host = host_g_depth1(c['depth0'].numpy(), c['depth1'].numpy(), c['flow'].numpy(), c['R0'].numpy(), c['t0'].numpy(), c['R1'].numpy(),
                         c['t1'].numpy(), c['K'].numpy(), c['mask'].numpy(), None, 0.7)
    assert np.array_equal(g1.numpy(), host)


# ---------------------------------------------------------------------------------------------------------------- 4. host restatement
def host_g_depth1(depth0, depth1, flow0, R0, t0, R1, t1, K, mask, clamp, gscale):
    """the single-term depth1 gradient (into a zeroed buffer) as the kernels define it, in numpy: fp32 taps and weights as
    bilin_zeros / tests/bitexact.py::sample_zeros spell them (no contraction), d1 and depth10 with the fused chains of
    bitexact.py, int64 sums of -sigma rint(w 2^32), then fp32(double(gs) (double(S) 2^-32))"""
    from tests import bitexact as B
    bs, _, h, w = depth0.shape
    ray = T.ORA['make_rays'](K, h, w).numpy()
    _, d1 = B.project(B.unproject(depth0, ray, R0, t0), K, R1, t1)
    d1 = d1.reshape(bs, h, w)
    u, v = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    px, py = B.add(flow0[:, 0], u), B.add(flow0[:, 1], v)
    raw = B.sub(d1, B.sample_zeros(depth1, px, py)[:, 0])
    m = mask.reshape(bs, h, w)
    live = m != 0
    if clamp is not None and clamp > 0:
        live &= ~(np.abs(raw) > f32(clamp))
    sigma = np.where(live, B.mul(m, np.sign(raw).astype(f32)), f32(0)).astype(np.int64)
    ix, iy = B._roundtrip(px, w), B._roundtrip(py, h)
    x0, y0 = np.floor(ix), np.floor(iy)
    wx, wy = B.sub(ix, x0), B.sub(iy, y0)
    ex, ey = B.sub(f32(1), wx), B.sub(f32(1), wy)
    x0i, y0i = np.clip(x0, -4, w + 4).astype(np.int64), np.clip(y0, -4, h + 4).astype(np.int64)
    S = np.zeros((bs, h, w), np.int64)
    bidx = np.broadcast_to(np.arange(bs)[:, None, None], (bs, h, w))
    for dx, dy, wt in ((0, 0, B.mul(ey, ex)), (1, 0, B.mul(ey, wx)), (0, 1, B.mul(wy, ex)), (1, 1, B.mul(wy, wx))):
        xi, yi = x0i + dx, y0i + dy
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (sigma != 0)
        q = np.rint(B.mul(wt, TWO32)).astype(np.int64)
        np.add.at(S, (bidx[ok], yi[ok], xi[ok]), -sigma[ok] * q[ok])
    gs = B.div(f32(gscale), B.add(f32(np.float64(m.sum(dtype=np.float64))), f32(1e-8)))
    out = (np.float64(gs) * (S.astype(np.float64) * 2.0 ** -32)).astype(f32)
    return (np.zeros((bs, h, w), f32) + out).reshape(bs, 1, h, w)


@pytest.mark.parametrize('mode', ['mf', 'sf'])
@pytest.mark.parametrize('bs_h_w', [(2, 2, 2), (3, 33, 41)])
def test_det_depth1_equals_host_restatement(bs_h_w, mode):
    bs, h, w = bs_h_w
    g = _input(bs, h, w)
    for (i, j) in ((0, 1), (1, 0)):
        ker, _, _, m, _ = _det_term(bs, h, w, i, j, mode)
        host = host_g_depth1(g['depth'][i].numpy(), g['depth'][j].numpy(), g['flow'][(i, j)].numpy(), g['R'][i].numpy(), g['t'][i].numpy(),
                             g['R'][j].numpy(), g['t'][j].numpy(), g['K'].numpy(), m, P.GEO_CLAMP if mode == 'sf' else None, 0.7)
        assert float(np.abs(host).max()) > 0
        diff = ker[2].numpy() != host
        assert np.array_equal(ker[2].numpy(), host), f'{mode} {bs_h_w} {i}->{j}: {int(diff.sum())} pixels differ from the restatement'


# ---------------------------------------------------------------------------------------------------------------- 5. det against atomic
def _within_golden(det, atomic, what):
    scale = float(atomic.abs().max())
    assert scale > 0
    d = P.dist(det.cpu(), atomic.cpu(), 2e-5 * scale, 1e-4)
    print(f'det vs atomic {what}: {d:.3e} of the golden tolerance')
    assert d <= 1.0, f'{what}: det and atomic differ by {d:.3e} x (2e-5 scale + 1e-4 |atomic|)'


@pytest.mark.parametrize('mode', ['mf', 'sf'])
@pytest.mark.parametrize('bs_h_w', P.GEO_SHAPES)
def test_det_equals_atomic_single(bs_h_w, mode):
    from depthinspace_amd import ops
    g = _input(*bs_h_w)
    for (i, j) in ((0, 1), (1, 0)):
        det = _dir_grads(g, i, j, mode)
        ops.set_geo_bwd_det(False)
        atomic = _dir_grads(g, i, j, mode)
        ops.set_geo_bwd_det(True)
        assert torch.equal(det[0], atomic[0]), 'the single-term g_depth0 is not the atomic form\'s bit for bit'
        _within_golden(det[1], atomic[1], f'g_depth1 {mode} {bs_h_w} {i}->{j}')


@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_det_equals_atomic_multi(mode):
    from depthinspace_amd import ops
    g = _input(3, 33, 41, 3)
    pairs = _pairs(mode)
    gvec = torch.linspace(0.5, 1.5, len(pairs))
    det = _all_grad(g, mode, pairs, gvec)
    ops.set_geo_bwd_det(False)
    atomic = _all_grad(g, mode, pairs, gvec)
    ops.set_geo_bwd_det(True)
    _within_golden(det, atomic, f'all-terms grad {mode}')


# ---------------------------------------------------------------------------------------------------------------- 6. edges
@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_det_empty_mask(mode):
    ker, ref, _, m, _ = _det_term(3, 33, 41, 0, 1, mode, 0.7, 2, True)
    assert float(m.sum()) == 0.0
    for k in (1, 2):
        assert bool(torch.isfinite(ker[k]).all()) and bool((ker[k] == 0).all()) and bool((ref[k] == 0).all())


def test_det_grad_accum():
    """two single-term calls (0 -> 1 and 1 -> 0) adding into one shared buffer per frame == the sum of the two calls run apart"""
    from depthinspace_amd import ops, lib
    g = _input(3, 33, 41)
    K, Ki = lib.host_floats(g['K'].reshape(-1)), lib.host_floats(g['Kinv'].reshape(-1))
    d = [g['depth'][k].cuda().requires_grad_(True) for k in (0, 1)]
    accs = [ops.GradAccum(), ops.GradAccum()]
    tot = 0
    for (i, j), gsc in (((0, 1), 0.7), ((1, 0), 1.1)):
        val, _ = ops.geo_loss_dir(d[i], d[j], g['flow'][(i, j)].cuda(), g['flow'][(j, i)].cuda(), g['amb'][i].cuda(), g['amb'][j].cuda(),
                                  g['pdepth'][j].cuda(), g['R'][i].cuda(), g['t'][i].cuda(), g['R'][j].cuda(), g['t'][j].cuda(), K, Ki, -1.0,
                                  (accs[i], accs[j]))
        tot = tot + val * gsc
    tot.backward()
    a0, a1 = _dir_grads(g, 0, 1, 'mf', 0.7)
    b1, b0 = _dir_grads(g, 1, 0, 'mf', 1.1)
    assert torch.equal(d[0].grad, a0 + b0) and torch.equal(d[1].grad, a1 + b1)


def test_det_rejects():
    from depthinspace_amd import lib
    q = lib.fn('dis_geo_loss_bwd_det_workspace')
    assert q(0, 3, 33, 41) == -1 and q(17, 3, 33, 41) == -1 and q(1, 0, 33, 41) == -1 and q(1, 3, 33, -1) == -1
    assert q(12, 4, 512, 432) == 12 * 4 * 512 * 432 * 12
    from depthinspace_amd import ops
    tab = (ops._GeoTerm * 17)()
    buf = torch.zeros(64, dtype=torch.float64).cuda()
    K = lib.host_floats(range(9))
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    rc = lib.fn('dis_geo_loss_bwd_multi_det')(p(tab), 17, p(K), p(K), -1.0, buf.data_ptr(), buf.data_ptr(), 3, 33, 41, buf.data_ptr(), None)
    assert rc == -2   # DIS_ERR_UNSUPPORTED
    with pytest.raises(lib.DisHipError):
        lib.call('dis_geo_loss_bwd_multi_det', tab, 1, K, K, -1.0, buf, buf, 3, 33, 41, None)   # no workspace


# ---------------------------------------------------------------------------------------------------------------- 7. / 8. the step
def _args(arch, bs):
    return argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic', architecture=arch,
                              epochs=1, warmup_epochs=150, train_batch_size=bs, max_disp=128)


def _make(arch, H=64, W=64, **kw):
    from depthinspace_amd import synth
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker, single_frame_worker, networks
    from depthinspace_amd.trainer import FlatAdam
    settings = synth.make_settings(H, W)
    torch.manual_seed(0)
    if arch == 'multi_frame':
        w = multi_frame_worker.Worker(_args(arch, 1), settings=settings, **kw)
        net = multi_frame_networks.FuseNet((H, W), settings.K, settings.baseline).cuda()
    else:
        w = single_frame_worker.Worker(_args(arch, 1), settings=settings, **kw)
        net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
    w.build_losses()
    w.current_epoch = 2
    opt = FlatAdam(net.parameters(), lr=1e-4)
    batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(settings, 1, 4, seed=4321, scene='bumps').items()}
    return w, net, opt, batch


def _geo_grad(w, arch, disp, flow):
    """gradient of the sum of the step's geometric terms wrt the disparities `disp` (tl, bs, 1, h, w)"""
    disp = disp.detach().clone().requires_grad_(True)
    depth = w.d2ds[0](disp)
    R, t, amb = w.data['R'], w.data['t'], w.data['ambient0']
    if arch == 'multi_frame':
        with torch.no_grad():
            primary_depth = w.d2ds[0](w.data['primary_disp'])
        allv = w.ge_losses[0].forward_all(depth, R, t, flow, amb, primary_depth)
    else:
        allv = w.ge_losses[0].forward_all(depth, R, t, flow, amb)
    assert allv is not None and len(allv) == 6
    sum(allv).backward()
    return disp.grad


@pytest.mark.parametrize('arch', ['multi_frame', 'single_frame'])
def test_det_step_repeats(arch):
    """tests/test_determinism_gpu.py's step with geo_bwd='det': the geometric terms' gradient wrt the network's disparity output
    repeats bit for bit; everything else keeps that test's bars (the GroupNorm statistics stay fp64 atomic sums)"""
    from depthinspace_amd import ops
    ops.set_geo_bwd_det(False)
    w, net, opt, batch = _make(arch, geo_bwd='det')
    assert ops.GEO_BWD_DET, "Worker(geo_bwd='det') did not select the order-free backward"
    runs = []
    for _ in range(4):
        w.copy_data(batch, device=w.train_device, requires_grad=False, train=True)
        opt.zero_grad()
        flow = w.read_optical_flow(True)
        out = w.net_forward(net, flow)
        losses = w.loss_forward(out, True, flow)
        sum(losses).backward()
        torch.cuda.synchronize()
        disp = (out[0] if isinstance(out, (list, tuple)) else out).detach().clone()
        runs.append((disp, np.array([float(l) for l in losses]), opt.flat_g.clone(), flow))
    d0, l0, g0, _ = runs[0]
    gmax = float(g0.abs().max())
    geo0 = _geo_grad(w, arch, d0, runs[0][3])
    assert float(geo0.abs().max()) > 0
    for d, l, g, flow in runs[1:]:
        assert float((d - d0).abs().max()) < 1e-5, 'forward pass does not repeat'
        np.testing.assert_allclose(l, l0, rtol=1e-6, atol=0)
        assert float((g - g0).abs().max()) / gmax < 1e-5
        # at the first run's disparities (a GroupNorm scale may move by one ulp between runs: not this kernel's business) ...
        assert torch.equal(_geo_grad(w, arch, d0, flow), geo0)
        # ... and at the run's own whenever the forward pass repeated bit for bit, which is the usual outcome
        if torch.equal(d, d0):
            assert torch.equal(_geo_grad(w, arch, d, flow), geo0)


def test_det_step_graph_equals_eager():
    """two captured steps (trainer.GraphedStep) in det mode against two eager ones: the entry points neither synchronise nor
    allocate, so the step captures; tolerance of tests/test_pipeline_gpu.py::test_worker_train_epoch_graph_equals_eager"""
    from depthinspace_amd.trainer import GraphedStep
    res = {}
    for mode in ('eager', 'graph'):
        w, net, opt, batch = _make('multi_frame', geo_bwd='det')
        st = GraphedStep(w, net, opt, batch, use_graph=(mode == 'graph'), strict=True)
        losses = []
        for _ in range(2):
            st.run(batch)
            losses.append(st.losses())
        torch.cuda.synchronize()
        assert st.mode == mode
        res[mode] = (opt.flat_p.clone(), np.array(losses))
    d = (res['eager'][0] - res['graph'][0]).abs()
    assert float(d.max()) <= 2.1e-4 * 2 and float(d.mean()) < 2e-6
    np.testing.assert_allclose(res['graph'][1], res['eager'][1], rtol=5e-3, atol=1e-5)
