"""GPU: dis_tsdf_integrate and dis_tsdf_mesh (csrc/tsdf.hip) against the numpy restatement tests/tsdf_ref.py - the volume against the
float64 integration, the mesh against the extraction of the device's own volume - plus the capacity limits, repeatability, graph
capture and the refusal of unsupported arguments.

Nothing here is a stored number.  The restatement runs in float32 and in float64 on the same input; float outputs may deviate from the
float64 values by tsdf_ref.tolerance = 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|), taken over the elements compared.  The
decisions of the integration (weight, the sign of tsdf) must equal the float64 ones except at the lattice points of tsdf_ref.exempt,
whose (lattice point, frame) pairs are capped at 0.1 % of all pairs (tests/test_tsdf_ref_cpu.py holds the restatement to the same
cap).  The mesh's topology (vid, cell, count, faces) hangs on comparisons of the volume's own float32 values only and must be exact."""
import ctypes

import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import tsdf_inputs as TI
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

SHAPES = list(TI.SHAPES)
_VOL = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _integrate(shape, kind, grid, value=True):
    from depthinspace_amd import ops
    a = TI.make_input(shape, kind)
    origin, voxel, trunc = TI.volume(shape, kind, grid)
    return ops.tsdf_integrate(_dev(a['disp']), _dev(a['R']), _dev(a['t']), a['K'], a['baseline'], _dev(a['value']) if value else None,
                              origin=origin, voxel=voxel, trunc=trunc, grid=grid)


def _volume(shape, kind, grid):
    """the device's own volume (device tensors) and its two extractions, computed once"""
    key = (shape, kind, grid)
    if key not in _VOL:
        vol = _integrate(shape, kind, grid)
        torch.cuda.synchronize()
        origin, voxel, _ = TI.volume(shape, kind, grid)
        e32, e64 = (tsdf_ref.extract(_np(vol[0]), _np(vol[1]), _np(vol[2]), origin, voxel, 1, dtype=dt) for dt in (np.float32, np.float64))
        _VOL[key] = (vol, e32, e64)
    return _VOL[key]


def _mesh(shape, kind, grid, **kw):
    from depthinspace_amd import ops
    vol = _volume(shape, kind, grid)[0]
    origin, voxel, _ = TI.volume(shape, kind, grid)
    return ops.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, **kw)


@pytest.mark.parametrize('kind', TI.KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=TI.shape_id)
def test_integrate_against_the_float64_restatement(shape, kind):
    for grid in TI.GRIDS:
        nx, ny, nz = grid
        r32, r64, ex, ex_pairs = TI.refs(shape, kind, grid)
        tsdf, weight, vvalue = _integrate(shape, kind, grid)
        torch.cuda.synchronize()
        share = ex_pairs.sum() / ex_pairs.size
        print(f'grid {grid}: exempt pairs {100 * share:.4f} %, exempt lattice points {int(ex.sum())} of {ex.size}')
        assert share <= 0.001
        m = ~ex
        w = _np(weight)
        assert w.shape == (nz, ny, nx) and w.dtype == np.uint8
        bad = (w != r64['weight']) & m
        print(f'  weight: {int(bad.sum())} points differ from float64 outside the exemption, {int((w != r32["weight"]).sum())} from float32 anywhere')
        assert not bad.any()
        g = _np(tsdf)
        assert g.shape == (nz, ny, nx) and g.dtype == np.float32
        bad = ((g < 0) != (r64['tsdf'] < 0)) & m
        print(f'  sign: {int(bad.sum())} points differ from float64 outside the exemption, '
              f'{int(((g < 0) != (r32["tsdf"] < 0)).sum())} from float32 anywhere')
        assert not bad.any()
        for k, got in (('tsdf', g), ('vvalue', _np(vvalue))):
            a32, a64 = r32[k].astype(np.float64), r64[k]
            allowed = tsdf_ref.tolerance(a32[m], a64[m])
            err = float(np.abs(got.astype(np.float64)[m] - a64[m]).max())
            print(f'  {k}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, equal to ref32 bit for bit: '
                  f'{bool(np.array_equal(got, r32[k].astype(np.float32)))}')
            assert np.isfinite(got).all() and err <= allowed, (k, err, allowed)
        # the comparison is not one of zeros
        if nx * ny * nz > 8:
            assert (r64['weight'][m] > 0).any() and (w[m] > 0).any() and (w[m] == 0).any()
            assert (r64['tsdf'][m] < 0).any() and (g[m] < 0).any()
            assert (r64['vvalue'][m] != 0).any() and (_np(vvalue)[m] != 0).any()


def test_integrate_without_a_value_plane():
    shape, kind, grid = SHAPES[1], 'bumps', TI.GRIDS[2]
    with_v = _integrate(shape, kind, grid)
    without = _integrate(shape, kind, grid, value=False)
    torch.cuda.synchronize()
    assert torch.equal(with_v[0].view(torch.int32), without[0].view(torch.int32)) and torch.equal(with_v[1], without[1])
    assert not bool(without[2].any()) and bool(with_v[2].any())


def _check_mesh(got, e32, e64, grid, label):
    nx, ny, nz = grid
    count = _np(got['count'])
    assert count.dtype == np.int32 and np.array_equal(count, e64['count']), (count, e64['count'])
    nv, nf = int(count[0]), int(count[1])
    vid = _np(got['vid'])
    assert vid.shape == (nz - 1, ny - 1, nx - 1) and vid.dtype == np.int32 and np.array_equal(vid, e64['vid'])
    assert np.array_equal(_np(got['cell'])[:nv], e64['cell']) and np.array_equal(_np(got['faces'])[:nf], e64['faces'])
    assert np.array_equal(e32['faces'], e64['faces']) and np.array_equal(e32['vid'], e64['vid'])
    assert np.array_equal(_np(got['views'])[:nv], e64['views']) and got['views'].dtype == torch.uint8
    for k in ('xyz', 'normal', 'value'):
        g = _np(got[k])[:nv]
        a32, a64 = e32[k].astype(np.float64), e64[k]
        allowed = tsdf_ref.tolerance(a32, a64)
        err = float(np.abs(g.astype(np.float64) - a64).max()) if nv else 0.0
        print(f'{label} {k}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, equal to ref32 bit for bit: '
              f'{bool(np.array_equal(g, e32[k].astype(np.float32)))}')
        assert np.isfinite(g).all() and err <= allowed, (k, err, allowed)
    return nv, nf


@pytest.mark.parametrize('kind', ['bumps', 'noise', 'holes'])
@pytest.mark.parametrize('shape', SHAPES, ids=TI.shape_id)
def test_mesh_of_the_devices_own_volume(shape, kind):
    for grid in TI.GRIDS:
        _, e32, e64 = _volume(shape, kind, grid)
        got = _mesh(shape, kind, grid, want_dense=True)
        torch.cuda.synchronize()
        nv, nf = _check_mesh(got, e32, e64, grid, f'grid {grid}')
        print(f'grid {grid}: {nv} vertices, {nf} triangles')
        assert got['xyz'].shape == (nv, 3) and got['faces'].shape == (nf, 3)
        if grid == (2, 2, 2):
            assert nf == 0
        elif min(grid) >= 17:
            assert nv > 0 and nf > 0      # the comparison is not one of empty meshes
    # a higher min_weight: fewer active cells, the same rules
    grid = TI.GRIDS[3]
    vol, _, _ = _volume(shape, kind, grid)
    origin, voxel, _ = TI.volume(shape, kind, grid)
    mw = shape[0]
    e32, e64 = (tsdf_ref.extract(_np(vol[0]), _np(vol[1]), _np(vol[2]), origin, voxel, mw, dtype=dt) for dt in (np.float32, np.float64))
    got = _mesh(shape, kind, grid, min_weight=mw, want_dense=True)
    torch.cuda.synchronize()
    _check_mesh(got, e32, e64, grid, f'min_weight {mw}')


def _raw_mesh(vol, origin, voxel, min_weight, vcap, fcap, bufs, grid, ws, nbytes, out='default'):
    from depthinspace_amd import lib
    O = lib.TsdfMeshOut()
    for f, _ in lib.TsdfMeshOut._fields_:
        setattr(O, f, bufs[f].data_ptr() if f in bufs else None)
    nx, ny, nz = grid
    lib.call('dis_tsdf_mesh', vol[0], vol[1], vol[2], lib.host_floats(origin) if origin is not None else None, voxel, min_weight, vcap, fcap,
             (ctypes.addressof(O) if out == 'default' else out), nx, ny, nz, ws, nbytes)


def _sentinel_bufs(vcap, fcap, pad=64):
    return {'xyz': torch.full((vcap * 3 + pad,), -7.0, device='cuda'), 'normal': torch.full((vcap * 3 + pad,), -7.0, device='cuda'),
            'value': torch.full((vcap + pad,), -7.0, device='cuda'), 'views': torch.full((vcap + pad,), 0x5a, dtype=torch.uint8, device='cuda'),
            'cell': torch.full((vcap + pad,), -7, dtype=torch.int32, device='cuda'),
            'faces': torch.full((fcap * 3 + pad,), -7, dtype=torch.int32, device='cuda'),
            'count': torch.full((2 + pad,), -7, dtype=torch.int32, device='cuda')}


@pytest.mark.parametrize('case', [(SHAPES[1], 'bumps', TI.GRIDS[2]), (SHAPES[2], 'noise', TI.GRIDS[3])], ids=['33x17x20', '40x40x48'])
def test_capacity(case):
    from depthinspace_amd import lib
    shape, kind, grid = case
    full = _mesh(shape, kind, grid)
    nv, nf = (int(v) for v in full['count'].tolist())
    assert nv > 8 and nf > 8
    fcap = nf - 5
    vcap = min(nv - 3, int(full['faces'][:fcap].max()) - 2)     # a few below: some triangle below fcap names a vertex >= vcap
    got = _mesh(shape, kind, grid, vcap=vcap, fcap=fcap)
    torch.cuda.synchronize()
    assert got['xyz'].shape == (vcap, 3) and got['faces'].shape == (fcap, 3) and torch.equal(got['count'], full['count'])
    for k in ('xyz', 'normal', 'value', 'views', 'cell'):
        assert torch.equal(got[k], full[k][:vcap]), k
    named = (full['faces'][:fcap] < vcap).all(dim=1)          # the triangles whose vertices were all written
    assert bool(named.any()) and not bool(named.all())
    assert torch.equal(got['faces'][named], full['faces'][:fcap][named])
    # the entry point itself, its outputs followed by sentinels: nothing is written at or beyond a cap, nor a triangle with a vertex >= vcap
    vol = _volume(shape, kind, grid)[0]
    origin, voxel, _ = TI.volume(shape, kind, grid)
    bufs = _sentinel_bufs(vcap, fcap)
    need = lib.fn('dis_tsdf_mesh_workspace')(*grid)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    _raw_mesh(vol, origin, voxel, 1, vcap, fcap, bufs, grid, ws, need)
    torch.cuda.synchronize()
    assert torch.equal(bufs['xyz'][:vcap * 3].view(vcap, 3), full['xyz'][:vcap]) and torch.equal(bufs['cell'][:vcap], full['cell'][:vcap])
    assert torch.equal(bufs['views'][:vcap], full['views'][:vcap]) and torch.equal(bufs['count'][:2], full['count'])
    faces = bufs['faces'][:fcap * 3].view(fcap, 3)
    assert torch.equal(faces[named], full['faces'][:fcap][named]) and bool((faces[~named] == -7).all())
    for k, used in (('xyz', vcap * 3), ('normal', vcap * 3), ('value', vcap), ('cell', vcap), ('faces', fcap * 3), ('count', 2)):
        assert bool((bufs[k][used:] == -7).all()), k
    assert bool((bufs['views'][vcap:] == 0x5a).all())
    # caps of zero: the counts alone
    zero = _mesh(shape, kind, grid, vcap=0, fcap=0)
    assert torch.equal(zero['count'], full['count']) and zero['xyz'].shape == (0, 3)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_repeatable_and_independent_of_the_workspace():
    from depthinspace_amd import lib
    shape, kind, grid = SHAPES[2], 'noise', TI.GRIDS[3]
    a, b = _integrate(shape, kind, grid), _integrate(shape, kind, grid)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    m1 = _mesh(shape, kind, grid, want_dense=True)
    m2 = _mesh(shape, kind, grid, want_dense=True)
    ws = torch.full((lib.fn('dis_tsdf_mesh_workspace')(*grid) + 64,), 0xff, dtype=torch.uint8, device='cuda')
    m3 = _mesh(shape, kind, grid, want_dense=True, workspace=ws)
    m4 = _mesh(shape, kind, grid)                     # the dense ids stay in the workspace
    torch.cuda.synchronize()
    assert int(m1['count'][1]) > 0
    for other in (m2, m3):
        for k in m1:
            assert torch.equal(_bits(m1[k]), _bits(other[k])), k
    assert set(m4) == set(m1) - {'vid'}
    for k in m4:
        assert torch.equal(_bits(m1[k]), _bits(m4[k])), k


@pytest.mark.parametrize('case', [(SHAPES[0], 'bumps', TI.GRIDS[2]), (SHAPES[1], 'holes', TI.GRIDS[3])], ids=['33x17x20', '40x40x48'])
def test_graph_capture_on_a_side_stream(case):
    from depthinspace_amd import ops, lib
    shape, kind, grid = case
    a = TI.make_input(shape, kind)
    origin, voxel, trunc = TI.volume(shape, kind, grid)
    vol = _integrate(shape, kind, grid)
    eager = _mesh(shape, kind, grid, want_dense=True)
    nv, nf = (int(v) for v in eager['count'].tolist())
    assert nv > 0 and nf > 0
    disp_d = torch.zeros(shape, device='cuda')
    R, t, val = _dev(a['R']), _dev(a['t']), _dev(a['value'])
    ws = torch.empty(lib.fn('dis_tsdf_mesh_workspace')(*grid), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        gvol = ops.tsdf_integrate(disp_d, R, t, a['K'], a['baseline'], val, origin=origin, voxel=voxel, trunc=trunc, grid=grid)
        out = ops.tsdf_mesh(gvol[0], gvol[1], gvol[2], origin, voxel, vcap=nv + 5, fcap=nf + 5, workspace=ws, want_dense=True)
    disp_d.copy_(_dev(a['disp']))                    # the capture executed nothing: the replay sees the disparities
    graph.replay()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    first_vol = [v.clone() for v in gvol]
    ws.fill_(0xff)                                   # the workspace needs no initialisation and carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    for gv in (first_vol, gvol):
        for x, y in zip(gv, vol):
            assert torch.equal(_bits(x), _bits(y))
    for res in (first, out):
        for k in eager:
            cut = {'faces': nf, 'count': 2, 'vid': None}.get(k, nv)
            x, y = (res[k], eager[k]) if cut is None else (res[k][:cut], eager[k][:cut])
            assert torch.equal(_bits(x), _bits(y)), k


def test_unsupported_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    inf, nan = float('inf'), float('nan')
    K = lambda a: np.array([[a['fx'], 0, a['cx']], [0, a['fy'], a['cy']], [0, 0, 1]], dtype=np.float64)
    # ---- dis_tsdf_integrate
    ok = dict(tl=2, h=16, w=24, nx=8, ny=6, nz=5, voxel=0.1, trunc=0.3, fx=100.0, fy=100.0, cx=12.0, cy=8.0, baseline=0.05, ox=-0.4, oy=-0.3,
              oz=0.8)
    bad = [dict(tl=0), dict(tl=5), dict(h=1), dict(w=1), dict(h=8193), dict(w=8193), dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025),
           dict(ny=1025), dict(nz=1025), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=inf), dict(voxel=nan), dict(trunc=0.0), dict(trunc=-1.0),
           dict(trunc=inf), dict(trunc=nan), dict(fx=0.0), dict(fx=-1.0), dict(fx=inf), dict(fx=nan), dict(fy=0.0), dict(fy=inf), dict(fy=nan),
           dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=inf), dict(baseline=nan), dict(cx=inf), dict(cx=nan), dict(cy=-inf),
           dict(cy=nan), dict(ox=inf), dict(oy=nan), dict(oz=-inf)]
    small = [kw for kw in bad if not (kw.get('h', 0) > 8192 or kw.get('w', 0) > 8192 or max(kw.get('nx', 0), kw.get('ny', 0), kw.get('nz', 0)) > 1024)]
    for kw in small + [dict(nx=1025)]:             # 1. the wrapper: nothing is allocated or launched
        a = dict(ok, **kw)
        disp = torch.ones(a['tl'], a['h'], a['w'], device='cuda')
        R, t = torch.eye(3, device='cuda').repeat(a['tl'], 1, 1), torch.zeros(a['tl'], 3, device='cuda')
        with pytest.raises(lib.DisHipError):
            ops.tsdf_integrate(disp, R, t, K(a), a['baseline'], origin=(a['ox'], a['oy'], a['oz']), voxel=a['voxel'], trunc=a['trunc'],
                               grid=(a['nx'], a['ny'], a['nz']))
    disp = torch.ones(2, 16, 24, device='cuda')
    R, t = torch.eye(3, device='cuda').repeat(2, 1, 1), torch.zeros(2, 3, device='cuda')
    with pytest.raises(RuntimeError):
        ops.tsdf_integrate(disp.cpu(), R, t, K(ok), 0.05, origin=(0, 0, 0), voxel=0.1, trunc=0.3, grid=(8, 6, 5))   # CPU tensors
    # 2. the entry point itself: sentinel-filled outputs stay untouched
    big = torch.ones(5 * 8193 * 24, device='cuda')     # disparities enough for every refused image shape
    Rb, tb = torch.eye(3, device='cuda').repeat(5, 1, 1), torch.zeros(5, 3, device='cuda')
    N = 1025 * 8 * 8
    outs = [torch.full((N,), -7.0, device='cuda'), torch.full((N,), 0x5a, dtype=torch.uint8, device='cuda'), torch.full((N,), -7.0, device='cuda')]

    def raw(a, skip=None):
        args = [big, Rb, tb, lib.host_floats([a['fx'], a['fy'], a['cx'], a['cy']]), a['baseline'], None,
                lib.host_floats([a['ox'], a['oy'], a['oz']]), a['voxel'], a['trunc'], outs[0], outs[1], outs[2]]
        if skip is not None:
            args[skip] = None
        lib.call('dis_tsdf_integrate', *args, a['tl'], a['h'], a['w'], a['nx'], a['ny'], a['nz'])

    for kw in bad:
        with pytest.raises(lib.DisHipError):
            raw(dict(ok, **kw))
    for skip in (0, 1, 2, 3, 6, 9, 10, 11):
        with pytest.raises(lib.DisHipError):
            raw(ok, skip=skip)
    torch.cuda.synchronize()
    assert bool((outs[0] == -7).all()) and bool((outs[1] == 0x5a).all()) and bool((outs[2] == -7).all())
    raw(ok)                                            # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    n = 8 * 6 * 5
    assert bool((outs[0][:n] != -7).all()) and bool((outs[0][n:] == -7).all()) and bool((outs[1][:n] <= 2).all()) and bool((outs[1][n:] == 0x5a).all())
    assert bool((outs[2][:n] == 0).all()) and bool((outs[2][n:] == -7).all())

    # ---- dis_tsdf_mesh
    okm = dict(nx=8, ny=6, nz=5, voxel=0.1, min_weight=1, vcap=16, fcap=16, ox=-0.4, oy=-0.3, oz=0.8)
    badm = [dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025), dict(ny=1025), dict(nz=1025), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=inf),
            dict(voxel=nan), dict(min_weight=0), dict(min_weight=5), dict(vcap=-1), dict(fcap=-1), dict(ox=inf), dict(oy=nan), dict(oz=-inf)]
    q = lib.fn('dis_tsdf_mesh_workspace')
    vol = (outs[0], outs[1], outs[2])                  # (the volume of the call above, followed by sentinels: large enough for 1025 x 8 x 8)
    vol_ok = tuple(v[:n].clone().view(5, 6, 8) for v in vol)
    for kw in badm:                                    # 1. the wrapper
        a = dict(okm, **kw)
        if set(kw) <= {'nx', 'ny', 'nz'}:
            assert q(a['nx'], a['ny'], a['nz']) == -1, kw
            v3 = tuple(v[:a['nx'] * a['ny'] * a['nz']].view(a['nz'], a['ny'], a['nx']) for v in vol)
        else:
            v3 = vol_ok
        with pytest.raises(lib.DisHipError):
            ops.tsdf_mesh(v3[0], v3[1], v3[2], (a['ox'], a['oy'], a['oz']), a['voxel'], min_weight=a['min_weight'], vcap=a['vcap'], fcap=a['fcap'])
    need = q(8, 6, 5)
    assert need > 0 and q(2, 2, 2) > 0 and q(1024, 1024, 1024) > 2 ** 32 and q(0, 8, 8) == -1 and q(8, -1, 8) == -1
    wsb = torch.empty(q(1024, 8, 8) + 16, dtype=torch.uint8, device='cuda')
    for w_ in (wsb[:need - 1], wsb[1:]):               # short; misaligned
        with pytest.raises(lib.DisHipError):
            ops.tsdf_mesh(vol_ok[0], vol_ok[1], vol_ok[2], (0, 0, 0), 0.1, vcap=4, fcap=4, workspace=w_)
    with pytest.raises(RuntimeError):
        ops.tsdf_mesh(vol_ok[0].cpu(), vol_ok[1].cpu(), vol_ok[2].cpu(), (0, 0, 0), 0.1)
    bufs = _sentinel_bufs(16, 16)                      # 2. the entry point itself

    def rawm(a, ws, nbytes, vol_=vol, **kw):
        _raw_mesh(vol_, [a['ox'], a['oy'], a['oz']], a['voxel'], a['min_weight'], a['vcap'], a['fcap'], kw.pop('bufs', bufs),
                  (a['nx'], a['ny'], a['nz']), ws, nbytes, **kw)

    for kw in badm:
        with pytest.raises(lib.DisHipError):
            rawm(dict(okm, **kw), wsb, wsb.numel())
    with pytest.raises(lib.DisHipError):
        rawm(okm, wsb[1:], wsb.numel() - 1)            # misaligned
    with pytest.raises(lib.DisHipError):
        rawm(okm, wsb, need - 1)                       # short
    with pytest.raises(lib.DisHipError):
        rawm(okm, None, need)                          # null
    with pytest.raises(lib.DisHipError):
        rawm(okm, wsb, wsb.numel(), out=None)
    for skip in range(3):
        with pytest.raises(lib.DisHipError):
            rawm(okm, wsb, wsb.numel(), vol_=tuple(None if i == skip else v for i, v in enumerate(vol)))
    for missing in ('count', 'xyz', 'views', 'faces'):
        with pytest.raises(lib.DisHipError):
            rawm(okm, wsb, wsb.numel(), bufs={k: v for k, v in bufs.items() if k != missing})
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == (0x5a if v.dtype == torch.uint8 else -7)).all()), k
    rawm(okm, wsb, wsb.numel(), vol_=vol_ok)           # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert bool((bufs['count'][:2] >= 0).all()) and bool((bufs['count'][2:] == -7).all())
