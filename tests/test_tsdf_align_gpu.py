"""GPU: dis_tsdf_align_poses (csrc/tsdf_align.hip) against the numpy restatement tests/tsdf_align_ref.py on the cases of
tests/tsdf_align_inputs.py - plus the exact degenerate case, repeatability, the independence of a view from the other views of its
call, the extent of what is written, invalid inputs, graph capture and the refusal of unsupported arguments.

Nothing here is a stored number.  The restatement runs on the same input with float32 per-pixel terms and float64 sums - what the
kernels do - and in float64.  The counts and the status must equal the float32 restatement exactly; the poses and the ratio
statistics may deviate from the float64 values by pose_ref.tolerance = 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|), each output
on its own.  tests/test_tsdf_align_ref_cpu.py holds, for every case kept, that the two restatements agree on the counts and that the
tolerance of R and t stays below 1e-4."""
import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import raycast_inputs as RI
from tests import tsdf_align_inputs as AI
from tests import tsdf_align_ref as AR
from tests import tsdf_inputs as TI

pytestmark = pytest.mark.gpu

_VOL = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ('R', 't', 'stats'))


def _volume(shape, kind, grid):
    key = (shape, kind, grid)
    if key not in _VOL:
        vol = RI.volume(shape, kind, grid)
        _VOL[key] = (_dev(vol['tsdf']), _dev(vol['weight']), vol['origin'], vol['voxel'], vol['trunc'])
    return _VOL[key]


def _align(shape, kind, grid, mode, params=None, views=None, **kw):
    from depthinspace_amd import ops
    a = TI.make_input(shape, kind)
    tsdf, weight, origin, voxel, trunc = _volume(shape, kind, grid)
    v = AI.views(shape, kind, grid, mode) if views is None else views
    iters, scale, damping = AI.case_params(shape, kind, grid) if params is None else params
    disp = kw.pop('disp', None)
    return ops.tsdf_align_poses(kw.pop('tsdf', tsdf), weight, origin, voxel, trunc, _dev(v['disp']) if disp is None else disp, a['K'], a['baseline'],
                                _dev(v['R_init']), _dev(v['t_init']), iters=iters, scale=AI.scale_of(scale, trunc), damping=damping, **kw)


@pytest.mark.parametrize('case', AI.kept(), ids=AI.case_id)
def test_align_against_the_float64_restatement(case):
    shape, kind, grid = case
    r32, r64 = AI.refs(*case)
    got = _align(*case, AI.mode_of(*case))
    torch.cuda.synchronize()
    g = {k: _np(v) for k, v in got.items()}
    nv = len(r64['R'])
    assert g['R'].shape == (nv, 3, 3) and g['t'].shape == (nv, 3) and g['stats'].shape == (nv, 8)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in g.values())
    assert np.array_equal(AI.counts(g), AI.counts(r32))             # pixels used in both passes, status, valid disparities
    for (name, a), (_, a32), (_, a64) in zip(AI.float_outputs(g), AI.float_outputs(r32), AI.float_outputs(r64)):
        allowed = AR.tolerance(a32, a64)
        err = float(np.abs(a.astype(np.float64) - a64).max())
        print(f'{name}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, max |device - ref32| '
              f'{float(np.abs(a.astype(np.float64) - a32.astype(np.float64)).max()):.3e}')
        assert err <= allowed, (name, err, allowed)
    v = AI.views(*case, AI.mode_of(*case))
    failed = g['stats'][:, 3] == 0
    if grid in AI.GRIDS:                                            # the comparison is not one of identities
        assert not failed.any() and float(np.abs(g['t'] - v['t_init']).max()) > 1e-5
    if grid == (2, 2, 2):
        assert failed.all()
    first = failed & (r32['steps'] == 0)                            # failed in the first pass: the start, bit for bit
    assert np.array_equal(g['R'][first], v['R_init'][first]) and np.array_equal(g['t'][first], v['t_init'][first])


def _slab(k0=6.0, grid=(12, 10, 14), h=16, w=24):
    """the analytic volume tsdf = clamp((k0 - k) / 3, -1, 1), constant in x and y, all weights 1, seen by an identity pose with a
    constant disparity that puts every pixel at lattice height 5.5: voxel 0.25, origin (-1.5, -1.25, 1), z = 2.375"""
    nx, ny, nz = grid
    k = np.arange(nz, dtype=np.float32)
    tsdf = np.broadcast_to(np.clip((np.float32(k0) - k) / np.float32(3), -1, 1)[:, None, None], (nz, ny, nx)).astype(np.float32)
    K = np.array([[40.0, 0, 11.5], [0, 40.0, 7.5], [0, 0, 1]], np.float32)
    baseline = 0.059375                                            # fx baseline = 2.375, disparity 1 -> z = 2.375
    disp = np.ones((1, h, w), np.float32)
    return dict(tsdf=tsdf, weight=np.ones((nz, ny, nx), np.uint8), origin=(-1.5, -1.25, 1.0), voxel=0.25, trunc=0.75, K=K, baseline=baseline,
                disp=disp, R=np.eye(3, dtype=np.float32)[None].copy(), t=np.zeros((1, 3), np.float32))


def test_a_volume_that_constrains_one_axis_fails_at_the_third_pivot_and_returns_its_start():
    from depthinspace_amd import ops
    s = _slab()
    assert float(np.float32(np.float32(s['K'][0, 0]) * np.float32(s['baseline']))) == 2.375
    ref, r64 = (AR.align(s['tsdf'], s['weight'], s['origin'], s['voxel'], s['trunc'], s['disp'], s['K'], s['baseline'], s['R'], s['t'], dtype=dt)
                for dt in (np.float32, np.float64))
    S = ref['sums'][0, 0]
    # every pixel is used; the x- and y-differences are exactly 0, so n = (0, 0, n2) and H_22 = H_33 = H_44 = 0 exactly
    assert S[29] == 16 * 24 and S[AR.hidx(2, 2)] == 0 and S[AR.hidx(3, 3)] == 0 and S[AR.hidx(4, 4)] == 0 and S[AR.hidx(0, 0)] > 0
    assert ref['stats'][0, 3] == 0 and ref['steps'][0] == 0
    pad = 16
    outs = [torch.full((n + pad,), float('nan'), device='cuda') for n in (9, 3, 8)]
    got = ops.tsdf_align_poses(_dev(s['tsdf']), _dev(s['weight']), s['origin'], s['voxel'], s['trunc'], _dev(s['disp']), s['K'], s['baseline'],
                               _dev(s['R']), _dev(s['t']))
    _raw(s, outs, 1, 16, 24)
    torch.cuda.synchronize()
    st = _np(got['stats'])[0]
    print('stats', st.tolist())
    assert np.array_equal(_np(got['R']), s['R']) and np.array_equal(_np(got['t']), s['t'])      # bit for bit
    assert st[3] == 0 and st[0] == 384 and st[4] == 384 and st[7] == 384
    assert st[5] > 0 and st[6] > 0 and st[1] == st[5] and st[2] == st[6]                       # the opening pass is still reported
    assert float(np.abs(st.astype(np.float64) - r64['stats'][0]).max()) <= AR.tolerance(ref['stats'], r64['stats'])
    for o, k, n in zip(outs, ('R', 't', 'stats'), (9, 3, 8)):      # every element written, nothing behind
        assert torch.equal(_bits(o[:n]), _bits(got[k].reshape(-1))) and bool(torch.isnan(o[n:]).all()), k


def _raw(s, outs, nv, h, w, ws=None, nbytes=None, **kw):
    """the entry point itself on the inputs dict s (numpy or device tensors; None: NULL)"""
    from depthinspace_amd import lib
    a = dict(s, iters=6, scale=s['trunc'] / 2 if s.get('trunc') else 1.0, damping=0.0, min_corr=64, min_weight=1)
    a.update(kw)
    dev = lambda x: _dev(x) if isinstance(x, np.ndarray) else x
    nz, ny, nx = a['grid'] if 'grid' in a else a['tsdf'].shape
    K = a['K']
    K4 = None if K is None else lib.host_floats([K[0][0], K[1][1], K[0][2], K[1][2]])
    if isinstance(ws, str):
        ws, nbytes = None, nbytes or 0
    elif ws is None:
        ws = torch.empty(lib.fn('dis_tsdf_align_workspace')(nv, h, w), dtype=torch.uint8, device='cuda')
    keep = [dev(a[k]) for k in ('tsdf', 'weight', 'disp', 'R', 't')]
    lib.call('dis_tsdf_align_poses', keep[0], keep[1], None if a['origin'] is None else lib.host_floats(a['origin']), a['voxel'], a['trunc'],
             a['min_weight'], keep[2], K4, a['baseline'], keep[3], keep[4], a['iters'], a['scale'], a['damping'], a['min_corr'], outs[0], outs[1],
             outs[2], nv, h, w, nx, ny, nz, ws, ws.numel() if nbytes is None else nbytes)


def test_repeatable_and_independent_of_workspace_and_layout():
    from depthinspace_amd import lib
    case = (AI.SHAPES[2], 'render', AI.GRIDS[1])
    v = AI.views(*case, 'track')
    a, b = _align(*case, 'track'), _align(*case, 'track')
    ws = torch.full((lib.fn('dis_tsdf_align_workspace')(4, 64, 96) + 64,), 0xff, dtype=torch.uint8, device='cuda')
    c = _align(*case, 'track', workspace=ws)
    d = _align(*case, 'track', workspace=ws)                          # ... nor of what the call before left in it
    e = _align(*case, 'track', disp=_dev(v['disp'][:, None]))          # (nv, 1, H, W)
    torch.cuda.synchronize()
    assert bool((a['stats'][:, 3] == 1).all())
    for other in (b, c, d, e):
        assert _same(a, other)
    assert bool((ws[-64:] == 0xff).all())


@pytest.mark.parametrize('case', [(AI.SHAPES[1], 'render', AI.GRIDS[0]), (AI.SHAPES[2], 'bumps', AI.GRIDS[2])], ids=AI.case_id)
def test_a_view_does_not_depend_on_the_other_views_of_the_call(case):
    tl = case[0][0]
    par = AI.PARAMS[0]
    many = _align(*case, 'many', params=par)
    one = _align(*case, 'one', params=par)
    track = _align(*case, 'track', params=par)
    torch.cuda.synchronize()
    for k in ('R', 't', 'stats'):
        assert torch.equal(_bits(one[k][0]), _bits(many[k][1])), k
    # the two copies of a frame start elsewhere and end elsewhere; the track's own call starts where neither does
    assert not torch.equal(many['R'][0], many['R'][tl]) and track['R'].shape[0] == tl and many['R'].shape[0] == 2 * tl + 1
    assert bool((many['stats'][:, 3] == 1).all())


@pytest.mark.parametrize('grid', [AI.GRIDS[0], AI.FAIL_GRIDS[0]], ids=RI.grid_id)
def test_every_output_element_is_written_and_nothing_behind(grid):
    case = (AI.SHAPES[1], 'holes', grid)                               # 24 x 40: tiles cut by both image edges
    a = TI.make_input(case[0], case[1])
    tsdf, weight, origin, voxel, trunc = _volume(*case)
    v = AI.views(*case, 'many')
    nv, (h, w), pad = len(v['disp']), case[0][1:], 64
    outs = [torch.full((n * nv + pad,), float('nan'), device='cuda') for n in (9, 3, 8)]
    s = dict(tsdf=tsdf, weight=weight, origin=origin, voxel=voxel, trunc=trunc, K=a['K'], baseline=a['baseline'], disp=v['disp'], R=v['R_init'],
             t=v['t_init'])
    _raw(s, outs, nv, h, w)
    ref = _align(*case, 'many', params=AI.PARAMS[0])
    torch.cuda.synchronize()
    for o, k, n in zip(outs, ('R', 't', 'stats'), (9, 3, 8)):
        assert torch.equal(_bits(o[:n * nv]), _bits(ref[k].reshape(-1))), k             # (a NaN left behind would differ)
        assert bool(torch.isnan(o[n * nv:]).all()), k
    assert bool((ref['stats'][:, 3] == (1 if grid in AI.GRIDS else 0)).all())


def test_invalid_disparities_and_unobserved_tsdf_are_not_read_into_the_result():
    case = (AI.SHAPES[1], 'holes', AI.GRIDS[1])
    tsdf, weight, origin, voxel, trunc = _volume(*case)
    v = AI.views(*case, 'track')
    base = _align(*case, 'track')
    disp = v['disp'].copy()
    bad = ~(np.isfinite(disp) & (disp > 0))
    assert bad.any()                                                # (the kind has holes)
    d_nan, d_mix = disp.copy(), disp.copy()
    d_nan[bad] = np.nan
    d_mix[bad] = np.where(np.arange(int(bad.sum())) % 3 == 0, -np.inf, np.where(np.arange(int(bad.sum())) % 3 == 1, -1.0, np.inf))
    t_nan = tsdf.clone()
    assert bool((weight == 0).any())
    t_nan[weight == 0] = float('nan')                               # a cell with an unobserved corner is never sampled
    outs = [_align(*case, 'track', disp=_dev(d_nan)), _align(*case, 'track', disp=_dev(d_mix)), _align(*case, 'track', tsdf=t_nan)]
    # knocking out a quarter of the valid pixels is seen
    d_less = disp.copy()
    d_less[:, ::2, ::2] = 0.0
    less = _align(*case, 'track', disp=_dev(d_less))
    torch.cuda.synchronize()
    for o in outs:
        assert _same(base, o)
    assert bool((less['stats'][:, 7] < base['stats'][:, 7]).all()) and bool((less['stats'][:, 0] < base['stats'][:, 0]).all())
    assert bool(torch.isfinite(less['R']).all()) and bool((base['stats'][:, 3] == 1).all())


@pytest.mark.parametrize('case', [(AI.SHAPES[0], 'bumps', AI.GRIDS[0]), (AI.SHAPES[2], 'render', AI.GRIDS[1])], ids=AI.case_id)
def test_graph_capture_on_a_side_stream(case):
    from depthinspace_amd import ops, lib
    shape, kind, grid = case
    a = TI.make_input(shape, kind)
    tsdf, weight, origin, voxel, trunc = _volume(*case)
    v = AI.views(*case, 'track')
    eager = _align(*case, 'track', params=AI.PARAMS[0])
    disp, R0, t0 = _dev(v['disp']), _dev(v['R_init']), _dev(v['t_init'])
    disp_c = torch.zeros_like(disp)                                    # no valid pixel at capture time
    ws = torch.empty(lib.fn('dis_tsdf_align_workspace')(*shape), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.tsdf_align_poses(tsdf, weight, origin, voxel, trunc, disp_c, a['K'], a['baseline'], R0, t0, workspace=ws)
    disp_c.copy_(disp)                                                 # the capture executed nothing: the replay sees the disparities
    graph.replay()
    torch.cuda.synchronize()
    first = {k: v_.clone() for k, v_ in out.items()}
    ws.fill_(0xff)                                                     # the workspace carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    assert bool((eager['stats'][:, 3] == 1).all())
    for res in (first, out):
        assert _same(eager, res)


def test_unsupported_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    inf, nan = float('inf'), float('nan')
    K = lambda a: np.array([[a['fx'], 0, a['cx']], [0, a['fy'], a['cy']], [0, 0, 1]], dtype=np.float64)
    ok = dict(nv=2, h=16, w=24, nx=12, ny=10, nz=14, voxel=0.25, trunc=0.75, min_weight=1, fx=40.0, fy=40.0, cx=11.5, cy=7.5, baseline=0.059375,
              ox=-1.5, oy=-1.25, oz=1.0, iters=6, scale=0.375, damping=0.0, min_corr=64)
    shapes = [dict(nv=0), dict(nv=65), dict(h=1), dict(w=1), dict(h=8193), dict(w=8193), dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025),
              dict(ny=1025), dict(nz=1025)]
    config = [dict(iters=0), dict(iters=65), dict(scale=0.0), dict(scale=-1.0), dict(scale=inf), dict(scale=nan), dict(scale=1e-30),
              dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=inf), dict(voxel=nan), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=inf), dict(trunc=nan),
              dict(damping=-1e-3), dict(damping=inf), dict(damping=nan), dict(min_corr=5), dict(min_weight=0), dict(min_weight=5), dict(fx=0.0),
              dict(fx=-1.0), dict(fx=inf), dict(fx=nan), dict(fy=0.0), dict(fy=inf), dict(fy=nan), dict(baseline=0.0), dict(baseline=-0.1),
              dict(baseline=inf), dict(baseline=nan), dict(cx=inf), dict(cx=nan), dict(cy=-inf), dict(cy=nan), dict(ox=inf), dict(oy=nan),
              dict(oz=-inf)]
    q = lib.fn('dis_tsdf_align_workspace')
    need = q(2, 16, 24)
    assert need > 0 and need % 16 == 0 and q(1, 2, 2) > 0 and q(64, 8192, 8192) > 0
    for kw in shapes[:6]:
        a = dict(ok, **kw)
        assert q(a['nv'], a['h'], a['w']) == -1, kw
    N = 1025 * 12 * 14
    k = (torch.arange(N, device='cuda') // 120).float()
    vol = (torch.clamp((6.0 - k) / 3.0, -1, 1).contiguous(), torch.ones(N, dtype=torch.uint8, device='cuda'))
    R65, t65 = torch.eye(3, device='cuda').repeat(65, 1, 1).contiguous(), torch.zeros(65, 3, device='cuda')
    disp = torch.ones(65 * 16 * 24, device='cuda')
    wsb = torch.empty(q(64, 16, 24) + 16, dtype=torch.uint8, device='cuda')
    for kw in shapes + config:                         # 1. the wrapper: nothing is allocated or launched
        a = dict(ok, **kw)
        if a['h'] > 8192 or a['w'] > 8192 or a['nv'] == 0:
            continue                                   # (the raw call below refuses them)
        n3 = a['nx'] * a['ny'] * a['nz']
        v3 = tuple(v[:n3].view(a['nz'], a['ny'], a['nx']) for v in vol)
        nv = a['nv']
        with pytest.raises(lib.DisHipError):
            ops.tsdf_align_poses(v3[0], v3[1], (a['ox'], a['oy'], a['oz']), a['voxel'], a['trunc'], disp[:nv * a['h'] * a['w']].view(nv, a['h'], a['w']),
                                 K(a), a['baseline'], R65[:nv], t65[:nv], iters=a['iters'], scale=a['scale'], damping=a['damping'],
                                 min_corr=a['min_corr'], min_weight=a['min_weight'])
    v_ok = tuple(v[:1680].view(14, 10, 12) for v in vol)
    d_ok = disp[:2 * 16 * 24].view(2, 16, 24)
    call_ok = lambda **kw: ops.tsdf_align_poses(kw.pop('tsdf', v_ok[0]), kw.pop('weight', v_ok[1]), (-1.5, -1.25, 1.0), 0.25, 0.75, kw.pop('disp', d_ok),
                                                K(ok), ok['baseline'], kw.pop('R', R65[:2]), kw.pop('t', t65[:2]), **kw)
    for w_ in (wsb[:need - 1], wsb[1:]):               # short; misaligned
        with pytest.raises(lib.DisHipError):
            call_ok(workspace=w_)
    for kw in (dict(tsdf=v_ok[0].cpu()), dict(disp=d_ok.cpu()), dict(R=R65[:2].cpu()), dict(weight=v_ok[1].cpu()), dict(disp=d_ok.double()),
               dict(weight=v_ok[1].float()), dict(tsdf=v_ok[0].transpose(0, 1)), dict(R=R65[:3]), dict(t=t65[:2, :2]), dict(disp=d_ok[0]),
               dict(workspace=wsb.float())):
        with pytest.raises(RuntimeError) as ei:
            call_ok(**kw)
        assert not isinstance(ei.value, lib.DisHipError), kw
    # 2. the entry point itself: NaN-filled outputs stay untouched
    outs = [torch.full((n * 2 + 16,), nan, device='cuda') for n in (9, 3, 8)]

    def raw(a, ws=wsb, nbytes=None, skip=None, **kw):
        s = dict(tsdf=vol[0], weight=vol[1], origin=[a['ox'], a['oy'], a['oz']], voxel=a['voxel'], trunc=a['trunc'], K=K(a), baseline=a['baseline'],
                 disp=disp, R=R65, t=t65, grid=(a['nz'], a['ny'], a['nx']))
        s.update(kw)
        o = list(outs)
        if skip is not None and skip < 3:
            o[skip] = None
        elif skip is not None:
            s[('tsdf', 'weight', 'disp', 'R', 't', 'origin', 'K')[skip - 3]] = None
        _raw(s, o, a['nv'], a['h'], a['w'], ws=ws, nbytes=nbytes, iters=a['iters'], scale=a['scale'], damping=a['damping'], min_corr=a['min_corr'],
             min_weight=a['min_weight'])

    def status(fn):
        with pytest.raises(lib.DisHipError) as ei:
            fn()
        return str(ei.value)

    for kw in shapes:
        assert 'bad shape' in status(lambda: raw(dict(ok, **kw))), kw
    for kw in config:
        assert 'unsupported' in status(lambda: raw(dict(ok, **kw))), kw
    for skip in range(10):                             # every pointer; NULL comes first, then the extents, then the rest
        assert 'null' in status(lambda: raw(dict(ok, nv=0, iters=0), skip=skip)), skip
    assert 'null' in status(lambda: raw(dict(ok, nv=0, iters=0), ws='null', nbytes=need))
    assert 'bad shape' in status(lambda: raw(dict(ok, nv=65, iters=0)))
    assert 'unsupported' in status(lambda: raw(ok, nbytes=need - 1))
    assert 'unsupported' in status(lambda: raw(ok, ws=wsb[1:], nbytes=wsb.numel() - 1))
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all())
    raw(ok)                                            # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    for o, n in zip(outs, (18, 6, 16)):
        assert bool(torch.isfinite(o[:n]).all()) and bool(torch.isnan(o[n:]).all())
    assert outs[2][4].item() == 384 and outs[2][7].item() == 384
