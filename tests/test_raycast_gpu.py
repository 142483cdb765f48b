"""GPU: dis_tsdf_raycast (csrc/raycast.hip) against the numpy restatement tests/raycast_ref.py, on the volumes of the float32
restatement of the integration (tests/raycast_inputs.py) - plus the equality of its two variants, the brick table, repeatability,
graph capture and the refusal of unsupported arguments.

Nothing here is a stored number.  The restatement runs in float32 and in float64 on the same input; the hit mask must equal the
float64 one except at the pixels of raycast_ref.exempt (capped at 0.5 % of every case's pixels, tests/test_raycast_ref_cpu.py holds
the restatement to the same cap), and over the other hit pixels the float outputs may deviate from the float64 values by
tsdf_ref.tolerance = 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|), taken over the elements compared."""
import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import raycast_inputs as RI
from tests import tsdf_inputs as TI
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

_DEV = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _inputs(shape, kind, grid):
    """the volume and the views of a case on the device, uploaded once"""
    key = (shape, kind, grid)
    if key not in _DEV:
        vol = RI.volume(shape, kind, grid)
        R, t = RI.views(shape, kind, grid)
        _DEV[key] = (_dev(vol['tsdf']), _dev(vol['weight']), _dev(vol['vvalue']), _dev(R), _dev(t))
    return _DEV[key]


def _cast(shape, kind, grid, step_voxels=1.0, **kw):
    from depthinspace_amd import ops
    a = TI.make_input(shape, kind)
    origin, voxel, _ = TI.volume(shape, kind, grid)
    tsdf, weight, vvalue, R, t = _inputs(shape, kind, grid)
    return ops.tsdf_raycast(tsdf, weight, vvalue, origin, voxel, kw.pop('R', R), kw.pop('t', t), a['K'], a['baseline'], size=shape[1:],
                            step=RI.step_of(voxel, step_voxels), **kw)


def _brick_table(ws, grid):
    """the state-2 counts of the bricks, as the header lays the workspace out"""
    nx, ny, nz = grid
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    nb = -(-(nx - 1) // 8) * -(-(ny - 1) // 8) * -(-(nz - 1) // 8)
    off = -(-cells // 16) * 16
    return ws[off:off + 4 * nb].view(torch.int32), ws[:cells]


def _check(got, refs, label):
    r32, r64, ex = refs
    m = ~ex
    disp = _np(got['disp'])
    assert disp.shape == r64['disp'].shape and disp.dtype == np.float32
    hit = disp > 0
    bad = (hit != r64['hit']) & m
    print(f'{label}: exempt {100 * ex.mean():.4f} %, hit {100 * r64["hit"].mean():.1f} %, {int(bad.sum())} pixels differ from float64 outside the '
          f'exemption, {int((hit != r32["hit"]).sum())} from float32 anywhere')
    assert ex.mean() <= 0.005 and not bad.any()
    mh = m & r64['hit']
    for k in ('disp', 'normal', 'value'):
        g = _np(got[k])
        assert g.shape == r64[k].shape and g.dtype == np.float32 and np.isfinite(g).all()
        sel = np.broadcast_to(mh[:, None], g.shape) if k == 'normal' else mh
        a32, a64 = r32[k].astype(np.float64)[sel], r64[k][sel]
        allowed = tsdf_ref.tolerance(a32, a64)
        err = float(np.abs(g.astype(np.float64)[sel] - a64).max()) if a64.size else 0.0
        print(f'  {k}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, equal to ref32 bit for bit: '
              f'{bool(np.array_equal(g, r32[k].astype(np.float32)))}')
        assert err <= allowed, (k, err, allowed)
        miss = np.broadcast_to((~hit)[:, None], g.shape) if k == 'normal' else ~hit
        assert not g[miss].any()                                  # a miss is 0 in all three outputs
    return hit


@pytest.mark.parametrize('grid', RI.GRIDS, ids=RI.grid_id)
@pytest.mark.parametrize('kind', RI.KINDS)
@pytest.mark.parametrize('shape', RI.SHAPES, ids=TI.shape_id)
def test_raycast_against_the_float64_restatement(shape, kind, grid):
    from depthinspace_amd import lib
    tl = shape[0]
    need = lib.fn('dis_tsdf_raycast_workspace')(*grid)
    for sv in RI.steps(shape, kind, grid):
        refs = RI.refs(shape, kind, grid, sv)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        got = _cast(shape, kind, grid, sv, workspace=ws)
        plain = _cast(shape, kind, grid, sv, variant=1)
        torch.cuda.synchronize()
        hit = _check(got, refs, f'grid {grid} step {sv:g}')
        for k in got:                                                 # the two variants give the same bits
            assert torch.equal(_bits(got[k]), _bits(plain[k])), k
        if min(grid) >= 17:                                           # the comparison is not one of zeros
            assert hit[:tl].any() and not hit.all() and (hit & ~refs[2]).any()
        if grid == (66, 64, 64):
            bricks, state = _brick_table(ws, grid)
            assert bricks.numel() == 9 * 8 * 8 and bool((bricks == 0).any()) and bool((bricks > 0).any())
            assert int(bricks.sum()) == int((state == 2).sum()) and int(state.max()) == 2
            print(f'  dead bricks {int((bricks == 0).sum())} of {bricks.numel()}')


@pytest.mark.parametrize('kind', ['bumps', 'holes'])
@pytest.mark.parametrize('shape', RI.SHAPES, ids=TI.shape_id)
def test_min_weight_of_the_track_length(shape, kind):
    grid, tl = RI.GRIDS[3], shape[0]
    refs = RI.refs(shape, kind, grid, 1.0, min_weight=tl)
    got = _cast(shape, kind, grid, min_weight=tl)
    plain = _cast(shape, kind, grid, min_weight=tl, variant=1)
    torch.cuda.synchronize()
    hit = _check(got, refs, f'min_weight {tl}')
    loose = RI.refs(shape, kind, grid, 1.0)[1]['hit']
    assert hit.any() and hit.sum() < loose.sum()
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(plain[k])), k


def _raw(vol, origin, voxel, min_weight, R, t, K4, baseline, step, variant, outs, nv, h, w, grid, ws, nbytes):
    from depthinspace_amd import lib
    nx, ny, nz = grid
    lib.call('dis_tsdf_raycast', vol[0], vol[1], vol[2], lib.host_floats(origin) if origin is not None else None, voxel, min_weight, R, t,
             lib.host_floats(K4) if K4 is not None else None, baseline, step, variant, outs[0], outs[1], outs[2], nv, h, w, nx, ny, nz, ws, nbytes)


@pytest.mark.parametrize('variant', [0, 1])
def test_every_output_element_is_written_and_nothing_behind(variant):
    from depthinspace_amd import lib
    shape, kind, grid = RI.SHAPES[1], 'holes', RI.GRIDS[2]           # 24 x 40: tiles cut by both image edges
    a = TI.make_input(shape, kind)
    origin, voxel, _ = TI.volume(shape, kind, grid)
    tsdf, weight, vvalue, R, t = _inputs(shape, kind, grid)
    nv, (h, w) = R.shape[0], shape[1:]
    n, pad = nv * h * w, 64
    outs = [torch.full((n + pad,), -7.0, device='cuda'), torch.full((3 * n + pad,), -7.0, device='cuda'), torch.full((n + pad,), -7.0, device='cuda')]
    need = lib.fn('dis_tsdf_raycast_workspace')(*grid)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    K4 = [float(a['K'][0, 0]), float(a['K'][1, 1]), float(a['K'][0, 2]), float(a['K'][1, 2])]
    _raw((tsdf, weight, vvalue), origin, voxel, 1, R, t, K4, a['baseline'], voxel, variant, outs, nv, h, w, grid, ws, need)
    ref = _cast(shape, kind, grid)
    torch.cuda.synchronize()
    for o, k, used in ((outs[0], 'disp', n), (outs[1], 'normal', 3 * n), (outs[2], 'value', n)):
        assert torch.equal(_bits(o[:used]), _bits(ref[k].reshape(-1))), k           # (a sentinel left behind would differ)
        assert bool((o[used:] == -7).all()), k
    assert bool((ref['disp'] > 0).any()) and bool((ref['disp'] == 0).any())


def test_repeatable_and_independent_of_the_workspace():
    from depthinspace_amd import lib
    shape, kind, grid = RI.SHAPES[2], 'noise', RI.GRIDS[3]
    a, b = _cast(shape, kind, grid), _cast(shape, kind, grid)
    ws = torch.full((lib.fn('dis_tsdf_raycast_workspace')(*grid) + 64,), 0xff, dtype=torch.uint8, device='cuda')
    c = _cast(shape, kind, grid, workspace=ws)
    d = _cast(shape, kind, grid, workspace=ws)                          # ... nor of what the call before left in it
    torch.cuda.synchronize()
    assert bool((a['disp'] > 0).any())
    for other in (b, c, d):
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(other[k])), k
    assert bool((ws[-64:] == 0xff).all())


@pytest.mark.parametrize('case', [(RI.SHAPES[0], 'bumps', RI.GRIDS[2]), (RI.SHAPES[1], 'holes', RI.GRIDS[3])], ids=['33x17x20', '40x40x48'])
def test_graph_capture_on_a_side_stream(case):
    from depthinspace_amd import ops, lib
    shape, kind, grid = case
    a = TI.make_input(shape, kind)
    origin, voxel, _ = TI.volume(shape, kind, grid)
    tsdf, weight, vvalue, R, t = _inputs(shape, kind, grid)
    eager = _cast(shape, kind, grid)
    assert bool((eager['disp'] > 0).any())
    tsdf_d = torch.ones_like(tsdf)                                     # an empty volume at capture time
    ws = torch.empty(lib.fn('dis_tsdf_raycast_workspace')(*grid), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.tsdf_raycast(tsdf_d, weight, vvalue, origin, voxel, R, t, a['K'], a['baseline'], size=shape[1:], workspace=ws)
    tsdf_d.copy_(tsdf)                                                 # the capture executed nothing: the replay sees the volume
    graph.replay()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    ws.fill_(0xff)                                                     # the workspace carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    for res in (first, out):
        for k in eager:
            assert torch.equal(_bits(res[k]), _bits(eager[k])), k


def test_unsupported_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    inf, nan = float('inf'), float('nan')
    K = lambda a: np.array([[a['fx'], 0, a['cx']], [0, a['fy'], a['cy']], [0, 0, 1]], dtype=np.float64)
    ok = dict(nv=2, h=16, w=24, nx=8, ny=6, nz=5, voxel=0.1, step=0.1, min_weight=1, variant=0, fx=100.0, fy=100.0, cx=12.0, cy=8.0,
              baseline=0.05, ox=-0.4, oy=-0.3, oz=0.8)
    bad = [dict(nv=0), dict(nv=65), dict(h=1), dict(w=1), dict(h=8193), dict(w=8193), dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025),
           dict(ny=1025), dict(nz=1025), dict(voxel=0.0, step=0.0), dict(voxel=-0.1), dict(voxel=inf), dict(voxel=nan), dict(fx=0.0),
           dict(fx=-1.0), dict(fx=inf), dict(fx=nan), dict(fy=0.0), dict(fy=inf), dict(fy=nan), dict(baseline=0.0), dict(baseline=-0.1),
           dict(baseline=inf), dict(baseline=nan), dict(cx=inf), dict(cx=nan), dict(cy=-inf), dict(cy=nan), dict(ox=inf), dict(oy=nan),
           dict(oz=-inf), dict(min_weight=0), dict(min_weight=5), dict(step=0.0124), dict(step=0.801), dict(step=0.0), dict(step=-0.1),
           dict(step=inf), dict(step=nan), dict(variant=-1), dict(variant=2),
           dict(voxel=3e38, step=3e38)]               # (the lattice's diagonal) voxel overflows: no bound on n
    q = lib.fn('dis_tsdf_raycast_workspace')
    need = q(8, 6, 5)
    assert need > 0 and q(2, 2, 2) > 0 and q(1024, 1024, 1024) > 2 ** 30 and q(0, 8, 8) == -1 and q(8, -1, 8) == -1 and q(8, 8, 1025) == -1
    N = 1025 * 8 * 8
    vol = (torch.ones(N, device='cuda'), torch.ones(N, dtype=torch.uint8, device='cuda'), torch.zeros(N, device='cuda'))
    vol[0][144:240] = -1.0                                             # the two farthest z layers of the 8 x 6 x 5 lattice lie behind a surface
    R65, t65 = torch.eye(3, device='cuda').repeat(65, 1, 1).contiguous(), torch.zeros(65, 3, device='cuda')
    wsb = torch.empty(q(1024, 8, 8) + 16, dtype=torch.uint8, device='cuda')
    for kw in bad:                                     # 1. the wrapper: nothing is allocated or launched
        a = dict(ok, **kw)
        if a['h'] > 8192 or a['w'] > 8192:
            continue                                   # (the wrapper would refuse them too; the raw call below does)
        if set(kw) <= {'nx', 'ny', 'nz'}:
            assert q(a['nx'], a['ny'], a['nz']) == -1, kw
        n3 = a['nx'] * a['ny'] * a['nz']
        v3 = tuple(v[:n3].view(a['nz'], a['ny'], a['nx']) for v in vol)
        with pytest.raises(lib.DisHipError):
            ops.tsdf_raycast(v3[0], v3[1], v3[2], (a['ox'], a['oy'], a['oz']), a['voxel'], R65[:a['nv']], t65[:a['nv']], K(a), a['baseline'],
                             size=(a['h'], a['w']), step=a['step'], min_weight=a['min_weight'], variant=a['variant'])
    v_ok = tuple(v[:240].view(5, 6, 8) for v in vol)
    for w_ in (wsb[:need - 1], wsb[1:]):               # short; misaligned
        with pytest.raises(lib.DisHipError):
            ops.tsdf_raycast(v_ok[0], v_ok[1], v_ok[2], (0, 0, 0), 0.1, R65[:2], t65[:2], K(ok), 0.05, size=(16, 24), workspace=w_)
    with pytest.raises(RuntimeError):
        ops.tsdf_raycast(v_ok[0].cpu(), v_ok[1].cpu(), v_ok[2].cpu(), (0, 0, 0), 0.1, R65[:2], t65[:2], K(ok), 0.05, size=(16, 24))
    # 2. the entry point itself: sentinel-filled outputs stay untouched
    n_out = 2 * 16 * 24
    outs = [torch.full((n_out + 64,), -7.0, device='cuda'), torch.full((3 * n_out + 64,), -7.0, device='cuda'),
            torch.full((n_out + 64,), -7.0, device='cuda')]

    def raw(a, ws=wsb, nbytes=None, skip=None, no_origin=False, no_k=False):
        v, rt, o = list(vol), [R65, t65], list(outs)
        if skip is not None:
            if skip < 3:
                v[skip] = None
            elif skip < 5:
                rt[skip - 3] = None
            else:
                o[skip - 5] = None
        _raw(v, None if no_origin else [a['ox'], a['oy'], a['oz']], a['voxel'], a['min_weight'], rt[0], rt[1],
             None if no_k else [a['fx'], a['fy'], a['cx'], a['cy']], a['baseline'], a['step'], a['variant'], o, a['nv'], a['h'], a['w'],
             (a['nx'], a['ny'], a['nz']), ws, wsb.numel() if nbytes is None else nbytes)

    for kw in bad:
        with pytest.raises(lib.DisHipError):
            raw(dict(ok, **kw))
    for skip in range(8):                              # every device pointer
        with pytest.raises(lib.DisHipError):
            raw(ok, skip=skip)
    for kw in (dict(no_origin=True), dict(no_k=True), dict(ws=None), dict(ws=wsb[1:], nbytes=wsb.numel() - 1), dict(nbytes=need - 1)):
        with pytest.raises(lib.DisHipError):
            raw(ok, **kw)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all())
    for variant in (0, 1):                             # the same call with nothing wrong goes through
        raw(dict(ok, variant=variant))
        torch.cuda.synchronize()
        assert bool((outs[0][:n_out] >= 0).all()) and bool((outs[0][:n_out] > 0).any())
        for o, used in zip(outs, (n_out, 3 * n_out, n_out)):
            assert bool((o[:used] != -7).all()) and bool((o[used:] == -7).all())
            o.fill_(-7.0)
