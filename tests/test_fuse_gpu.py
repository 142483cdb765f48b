"""GPU: dis_fuse_track (csrc/fuse.hip) against the float64 numpy restatement tests/fuse_ref.py - the dense maps, the fused points and
normals, the counts - plus the compaction held exactly against the device's own dense maps, the capacity limit, repeatability, graph
capture and the refusal of unsupported arguments.

Nothing here is a stored number.  The restatement runs in float32 and in float64 on the same input; float outputs may deviate from the
float64 values by fuse_ref.tolerance = 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|), taken over the pixels compared.  Decisions
(views, seen, keep) must equal the float64 ones except at the pixels of fuse_ref.exempt - a residual within the band of the tolerance,
a projection within the band of an image edge or of a cell boundary next to a hole, a `seen` flag the two dtypes already take
differently - and those are capped at 1 % of the pairs (tests/test_fuse_ref_cpu.py holds the restatements to the same cap)."""
import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import fuse_inputs as FI
from tests import fuse_ref

pytestmark = pytest.mark.gpu

BIG = (1, 4, 272, 248)   # 1054 blocks of 256 pixels: more than the scan workgroup covers in one pass of 1024


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(shape, kind, tol=0.01, min_views=2, layout5=False, value=True, **kw):
    from depthinspace_amd import ops
    a = FI.make_input(shape, kind)
    disp, val = _dev(a['disp']), _dev(a['value'])
    if layout5:
        disp, val = disp[:, :, None], val[:, :, None]
    return ops.fuse_track(disp, _dev(a['R']), _dev(a['t']), a['K'], a['baseline'], val if value else None, tol=tol, min_views=min_views, **kw)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('kind', FI.INPUTS)
@pytest.mark.parametrize('shape', FI.SHAPES, ids=FI.shape_id)
def test_against_the_float64_restatement(shape, kind):
    n, tl, H, W = shape
    for pi in range(len(FI.PARAMS)):
        tol, mv = FI.params(shape, pi)
        r32, r64, ex, ex_pairs = FI.refs(shape, kind, pi)
        got = _run(shape, kind, tol, mv, want_dense=True)
        torch.cuda.synchronize()
        share = ex_pairs.sum() / FI.pair_count(shape)
        print(f'params {pi}: exempt pairs {100 * share:.4f} %, exempt pixels {ex.sum()}')
        assert share <= 0.01
        m = ~ex
        for k in ('views', 'seen', 'keep'):
            g = _np(got[k])
            assert g.shape == (n, tl, H, W) and g.dtype == np.uint8
            bad = (g != r64[k].astype(np.uint8)) & m
            print(f'  {k}: {int(bad.sum())} pixels differ from float64 outside the exemption, {int((g != r32[k].astype(np.uint8)).sum())} '
                  f'from float32 anywhere')
            assert not bad.any(), (k, int(bad.sum()))
        for k, rk in (('resid', 'resid'), ('point', 'point'), ('dnormal', 'normal')):
            g = _np(got[k]).astype(np.float64)
            a32, a64 = r32[rk].astype(np.float64), r64[rk]
            if g.ndim == 5:
                g, a32, a64 = (np.moveaxis(x, 2, -1) for x in (g, a32, a64))
            allowed = fuse_ref.tolerance(a32[m], a64[m])
            err = float(np.abs(g[m] - a64[m]).max()) if m.any() else 0.0
            print(f'  {k}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, equal to ref32 bit for bit: '
                  f'{bool(np.array_equal(g[m].astype(np.float32), a32[m].astype(np.float32)))}')
            assert np.isfinite(g[m]).all() and err <= allowed, (k, err, allowed)
        count = _np(got['count'])
        assert count.shape == (n,) and count.dtype == np.int32
        assert int(np.abs(count.astype(np.int64) - r64['count']).sum()) <= int(ex.sum())
        # the comparison is not one of zeros
        if H * W > 4:
            assert r64['seen'].any() and bool(got['seen'].any())
            if not (kind == 'scaled' and mv == tl):
                assert r64['keep'].any() and bool(got['keep'].any())


def _check_compaction(got, a, shape, cap=None):
    n, tl, H, W = shape
    keep = _np(got['keep']).astype(bool)
    count = _np(got['count'])
    assert np.array_equal(count, keep.reshape(n, -1).sum(1))
    total = int(count.sum())
    m = total if cap is None else min(total, cap)
    want_src = np.flatnonzero(keep.reshape(-1))[:m]
    src = _np(got['src'])[:m].astype(np.int64)
    assert np.all(np.diff(src) > 0) and np.array_equal(src, want_src)
    flat = lambda t: np.moveaxis(_np(t), 2, -1).reshape(-1, 3)
    assert np.array_equal(_np(got['xyz'])[:m].view(np.uint32), flat(got['point'])[src].view(np.uint32))
    assert np.array_equal(_np(got['normal'])[:m].view(np.uint32), flat(got['dnormal'])[src].view(np.uint32))
    val = a['value'].reshape(-1)[src] if a is not None else np.zeros(m, np.float32)
    assert np.array_equal(_np(got['value'])[:m].view(np.uint32), val.view(np.uint32))
    return total


@pytest.mark.parametrize('shape', FI.SHAPES + [BIG], ids=FI.shape_id)
def test_compaction_is_exact(shape):
    for kind, tol, mv in (('holes', 0.01, 2), ('noise', 0.002, 1)):
        got = _run(shape, kind, tol, mv, want_dense=True)
        torch.cuda.synchronize()
        total = _check_compaction(got, FI.make_input(shape, kind), shape)
        assert total > 0 or shape[2] * shape[3] <= 4
    got = _run(shape, 'noise', 0.002, 1, value=False, want_dense=True)
    _check_compaction(got, None, shape)


@pytest.mark.parametrize('shape', [FI.SHAPES[2], FI.SHAPES[3]], ids=FI.shape_id)
def test_capacity(shape):
    from depthinspace_amd import ops, lib
    n, tl, H, W = shape
    a = FI.make_input(shape, 'bumps')
    full = _run(shape, 'bumps', want_dense=True)
    total = int(full['count'].sum().item())
    assert total > 5
    cap = total - 5
    got = _run(shape, 'bumps', want_dense=True, cap=cap)
    torch.cuda.synchronize()
    assert got['xyz'].shape == (cap, 3) and got['src'].shape == (cap,)
    assert torch.equal(got['count'], full['count'])
    for k in ('xyz', 'normal', 'value', 'src'):
        assert torch.equal(got[k], full[k][:cap]), k
    _check_compaction(got, a, shape, cap=cap)
    # the entry point itself, its outputs followed by a sentinel: nothing is written past cap
    pad = 64
    bufs = {'xyz': torch.full((cap * 3 + pad,), -7.0, device='cuda'), 'normal': torch.full((cap * 3 + pad,), -7.0, device='cuda'),
            'value': torch.full((cap + pad,), -7.0, device='cuda'), 'src': torch.full((cap + pad,), -7, dtype=torch.int32, device='cuda'),
            'count': torch.full((n + pad,), -7, dtype=torch.int32, device='cuda')}
    dense = {k: torch.empty((n, tl, H, W), dtype=torch.uint8, device='cuda') for k in ('views', 'seen', 'keep')}
    dense['resid'] = torch.empty((n, tl, H, W), device='cuda')
    O = lib.FuseOut()
    for f, _ in lib.FuseOut._fields_:
        setattr(O, f, bufs[f].data_ptr() if f in bufs else (dense[f].data_ptr() if f in dense else None))
    import ctypes
    need = lib.fn('dis_fuse_workspace')(n, tl, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    lib.call('dis_fuse_track', _dev(a['disp']), _dev(a['R']), _dev(a['t']), lib.host_floats([a['K'][0, 0], a['K'][1, 1], a['K'][0, 2], a['K'][1, 2]]),
             float(a['baseline']), None, 0.01, 2, cap, ctypes.addressof(O), n, tl, H, W, ws, need)
    torch.cuda.synchronize()
    assert torch.equal(bufs['xyz'][:cap * 3].view(cap, 3), full['xyz'][:cap]) and torch.equal(bufs['src'][:cap], full['src'][:cap])
    assert torch.equal(bufs['count'][:n], full['count']) and not bool(bufs['value'][:cap].any())
    for k, used in (('xyz', cap * 3), ('normal', cap * 3), ('value', cap), ('src', cap), ('count', n)):
        assert bool((bufs[k][used:] == -7).all()), k


def test_repeatable_and_independent_of_workspace_and_layout():
    from depthinspace_amd import lib
    shape = FI.SHAPES[3]
    n, tl, H, W = shape
    a = _run(shape, 'noise', want_dense=True)
    b = _run(shape, 'noise', want_dense=True)
    ws = torch.full((lib.fn('dis_fuse_workspace')(n, tl, H, W) + 64,), 0xff, dtype=torch.uint8, device='cuda')
    c = _run(shape, 'noise', want_dense=True, workspace=ws)
    d = _run(shape, 'noise', want_dense=True, layout5=True)
    e = _run(shape, 'noise')                                   # the dense point and normal stay in the workspace
    torch.cuda.synchronize()
    total = int(a['count'].sum().item())
    assert total > 0
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    for other in (b, c, d):
        for k in a:
            x, y = (a[k], other[k]) if k not in ('xyz', 'normal', 'value', 'src') else (a[k][:total], other[k][:total])
            assert torch.equal(bits(x), bits(y)), k
    assert set(e) == {'xyz', 'normal', 'value', 'src', 'count'}
    for k in e:
        assert torch.equal(bits(e[k][:total] if k != 'count' else e[k]), bits(a[k][:total] if k != 'count' else a[k])), k


@pytest.mark.parametrize('shape', [FI.SHAPES[1], FI.SHAPES[2]], ids=FI.shape_id)
def test_graph_capture_on_a_side_stream(shape):
    from depthinspace_amd import ops, lib
    n, tl, H, W = shape
    a = FI.make_input(shape, 'bumps')
    eager = _run(shape, 'bumps', want_dense=True)
    total = int(eager['count'].sum().item())
    assert total > 0
    disp_d = torch.zeros(shape, device='cuda')
    R, t, val = _dev(a['R']), _dev(a['t']), _dev(a['value'])
    ws = torch.empty(lib.fn('dis_fuse_workspace')(n, tl, H, W), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.fuse_track(disp_d, R, t, a['K'], a['baseline'], val, workspace=ws, want_dense=True)
    disp_d.copy_(_dev(a['disp']))                    # the capture executed nothing: the replay sees the disparities
    graph.replay()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    ws.fill_(0xff)                                   # the workspace needs no initialisation and carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    for res in (first, out):
        for k in eager:
            cut = (lambda x: x[:total]) if k in ('xyz', 'normal', 'value', 'src') else (lambda x: x)
            x, y = cut(res[k]), cut(eager[k])
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k


def test_unsupported_arguments_are_refused_before_any_launch():
    import ctypes
    from depthinspace_amd import ops, lib
    inf, nan = float('inf'), float('nan')
    ok = dict(n=1, tl=2, h=16, w=24, tol=0.01, min_views=2, fx=100.0, fy=100.0, baseline=0.05, cap=10)
    bad = [dict(tl=1), dict(tl=5), dict(h=1), dict(w=1), dict(h=8193), dict(w=8193), dict(n=0), dict(tol=0.0), dict(tol=1.0), dict(tol=-0.1),
           dict(tol=nan), dict(tol=inf), dict(min_views=0), dict(min_views=3), dict(fx=0.0), dict(fx=-1.0), dict(fx=inf), dict(fx=nan),
           dict(fy=0.0), dict(fy=inf), dict(fy=nan), dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=inf), dict(baseline=nan),
           dict(cap=-1)]
    K = lambda a: np.array([[a['fx'], 0, 10.0], [0, a['fy'], 8.0], [0, 0, 1]], dtype=np.float64)
    # 1. the wrapper: nothing is allocated or launched
    for kw in bad:
        a = dict(ok, **kw)
        disp = torch.ones(a['n'], a['tl'], a['h'], a['w'], device='cuda')
        R = torch.eye(3, device='cuda').repeat(a['n'], a['tl'], 1, 1)
        t = torch.zeros(a['n'], a['tl'], 3, device='cuda')
        with pytest.raises(lib.DisHipError):
            ops.fuse_track(disp, R, t, K(a), a['baseline'], tol=a['tol'], min_views=a['min_views'], cap=a['cap'])
    disp = torch.ones(1, 2, 16, 24, device='cuda')
    R, t = torch.eye(3, device='cuda').repeat(1, 2, 1, 1), torch.zeros(1, 2, 3, device='cuda')
    need = lib.fn('dis_fuse_workspace')(1, 2, 16, 24)
    ws = torch.empty(need + 16, dtype=torch.uint8, device='cuda')
    for w_ in (ws[:need - 1], ws[1:]):                # short; misaligned
        with pytest.raises(lib.DisHipError):
            ops.fuse_track(disp, R, t, K(ok), 0.05, workspace=w_)
    with pytest.raises(RuntimeError):
        ops.fuse_track(disp.cpu(), R, t, K(ok), 0.05)  # CPU tensors: the HIP path is the only path
    # 2. the entry point itself: sentinel-filled outputs stay untouched
    big = torch.ones(5 * 8193 * 24, device='cuda')    # disparities enough for every refused shape
    Rb, tb = torch.eye(3, device='cuda').repeat(5, 1, 1), torch.zeros(5, 3, device='cuda')
    outs = {k: torch.full((5 * 8193 * 24,), 0x5a, dtype=torch.uint8, device='cuda') for k in ('views', 'seen', 'keep')}
    outs.update({k: torch.full((5 * 8193 * 24,), -7.0, device='cuda') for k in ('resid',)})
    outs.update({k: torch.full((64,), -7.0, device='cuda') for k in ('xyz', 'normal', 'value')})
    outs.update({k: torch.full((64,), -7, dtype=torch.int32, device='cuda') for k in ('src', 'count')})
    O = lib.FuseOut()
    for f, _ in lib.FuseOut._fields_:
        setattr(O, f, outs[f].data_ptr() if f in outs else None)
    wsb = torch.empty(lib.fn('dis_fuse_workspace')(1, 4, 8192, 24) + 16, dtype=torch.uint8, device='cuda')

    def raw(a, workspace, nbytes, out=O):
        lib.call('dis_fuse_track', big, Rb, tb, lib.host_floats([a['fx'], a['fy'], 10.0, 8.0]), a['baseline'], None, a['tol'], a['min_views'],
                 a['cap'], ctypes.addressof(out) if out is not None else None, a['n'], a['tl'], a['h'], a['w'], workspace, nbytes)

    for kw in bad:
        with pytest.raises(lib.DisHipError):
            raw(dict(ok, **kw), wsb, wsb.numel())
    with pytest.raises(lib.DisHipError):
        raw(ok, wsb[1:], wsb.numel() - 1)              # misaligned
    with pytest.raises(lib.DisHipError):
        raw(ok, wsb, need - 1)                         # short
    with pytest.raises(lib.DisHipError):
        raw(ok, None, need)                            # null
    with pytest.raises(lib.DisHipError):
        raw(ok, wsb, wsb.numel(), out=None)
    P = lib.FuseOut()
    for f, _ in lib.FuseOut._fields_:
        setattr(P, f, outs[f].data_ptr() if f in outs and f != 'resid' else None)
    with pytest.raises(lib.DisHipError):
        raw(ok, wsb, wsb.numel(), out=P)               # a mandatory dense map is missing
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == (0x5a if v.dtype == torch.uint8 else -7)).all()), k
    raw(ok, wsb, wsb.numel())                          # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    px = 2 * 16 * 24
    assert int(outs['count'][0]) >= 0 and bool((outs['count'][1:] == -7).all())
    assert bool(((outs['views'][:px] == 1) | (outs['views'][:px] == 2)).all()) and bool((outs['views'][px:] == 0x5a).all())
    q = lib.fn('dis_fuse_workspace')
    assert q(1, 2, 16, 24) > 0 and q(1, 2, 2, 2) > 0 and q(3, 4, 8192, 8192) > 0
    for kw in bad:
        if set(kw) <= {'n', 'tl', 'h', 'w'}:
            a = dict(ok, **kw)
            assert q(a['n'], a['tl'], a['h'], a['w']) == -1, kw
    assert q(1 << 20, 4, 64, 64) == -1 and q(8, 4, 8192, 8192) == -1 and q(-1, 2, 16, 24) == -1
