"""GPU: dis_dense_flow (csrc/flow.hip) against the float64 numpy restatement tests/flow_ref.py, stage by stage - the normalised
pyramid, the warped image and the derivatives, the flow after every level, the result - plus accuracy against the exact flow,
repeatability, graph capture and the refusal of unsupported arguments.

The tolerance is not a stored number: the restatement runs in float32 and in float64 on the same input, and the device may deviate
from the float64 values, per stage, by 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|) (flow_ref.stage_tolerance): 16 for the
device's right to order commutative sums differently from numpy, the second term a floor of a few ulps where both references agree."""
import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import flow_ref

pytestmark = pytest.mark.gpu

# (n, tl, H, W): odd extents, narrower than a tile plus halo in one direction; two tracks, three frames; all 12 pairs, several tiles
# and levels; a single level smaller than the halo; taller than wide with tile edges off the image edge
SHAPES = [(1, 2, 37, 83), (2, 3, 24, 40), (1, 4, 96, 160), (1, 2, 15, 15), (1, 2, 130, 70)]
INPUTS = ['bumps', 'plane', 'const', 'gain']
# the second set: 13 steps are no multiple of the 8 a launch runs; min_size 4 adds levels; its debug level is the coarsest
PARAMS = [dict(alpha=1.0, warps=3, iters=64, min_size=8), dict(alpha=0.5, warps=1, iters=13, min_size=4)]

_INPUT, _REF = {}, {}


def _debug_level(shape, pi):
    return 0 if pi == 0 else len(flow_ref.level_sizes(shape[2], shape[3], PARAMS[pi]['min_size'])) - 1


def _input(shape, kind):
    """(frames (n, tl, H, W) float32, the batch of synth.make_batch or None)"""
    key = (shape, kind)
    if key not in _INPUT:
        from depthinspace_amd import synth
        n, tl, H, W = shape
        batch = None
        if kind == 'const':
            fr = np.broadcast_to((0.2 + 0.1 * np.arange(n * tl, dtype=np.float32)).reshape(n, tl, 1, 1), shape)
        else:
            batch = synth.make_batch(synth.make_settings(H, W), n, tl=tl, seed=7, scene='plane' if kind == 'plane' else 'bumps',
                                     motion=0.1, with_primary=False)
            fr = batch['ambient0'][:, :, 0].copy()
            if kind == 'gain':
                fr[:, 1::2] = 1.7 * fr[:, 1::2] + 0.1
        _INPUT[key] = (np.ascontiguousarray(fr, dtype=np.float32), batch)
    return _INPUT[key]


def _ref(shape, kind, pi):
    """(float32 restatement, float64 restatement), computed once per input and never changed"""
    key = (shape, kind, pi)
    if key not in _REF:
        fr = _input(shape, kind)[0]
        _REF[key] = tuple(flow_ref.dense_flow(fr, dtype=dt, debug_level=_debug_level(shape, pi), **PARAMS[pi])
                          for dt in (np.float32, np.float64))
    return _REF[key]


def _run(shape, kind, pi, **kw):
    from depthinspace_amd import ops
    return ops.dense_flow(torch.from_numpy(_input(shape, kind)[0]).cuda(), **PARAMS[pi], **kw)


def _close(got, r32, r64, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    tol = flow_ref.stage_tolerance(r32, r64)
    err = float(np.abs(got - r64).max())
    bits = bool(np.array_equal(got.astype(np.float32), r32))
    print(f'{what}: max |device - ref64| {err:.3e}, allowed {tol:.3e}, max |ref32 - ref64| {np.abs(r32 - r64).max():.3e}, '
          f'equal to ref32 bit for bit: {bits}')
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize('kind', INPUTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_every_stage_is_within_the_reference_tolerance(shape, kind):
    n, tl, H, W = shape
    for pi in range(len(PARAMS)):
        r32, r64 = _ref(shape, kind, pi)
        flow, dbg = _run(shape, kind, pi, want_debug=True, debug_level=_debug_level(shape, pi))
        torch.cuda.synchronize()
        assert flow.shape == (n, tl * tl, 2, H, W) and flow.dtype == torch.float32
        assert len(dbg['pyr']) == len(r64['pyr']) == len(dbg['levels'])
        for k in range(len(r64['pyr'])):
            _close(dbg['pyr'][k], r32['pyr'][k], r64['pyr'][k], f'params {pi} pyramid level {k}')
        for c, name in enumerate(('warped', 'Ix', 'Iy', 'It')):
            _close(dbg['warp'][c], r32['warp'][c], r64['warp'][c], f'params {pi} {name} at level {_debug_level(shape, pi)}')
        for k in range(len(r64['pyr']) - 1, -1, -1):
            _close(dbg['levels'][k], r32['levels'][k], r64['levels'][k], f'params {pi} flow after level {k}')
        _close(flow, r32['flow'], r64['flow'], f'params {pi} flow')
        for i in range(tl):
            assert not bool(flow[:, i * tl + i].any())              # the diagonal
        if kind == 'const':
            assert not bool(flow.any())
        elif pi == 0:
            assert float(np.abs(r64['flow']).max()) > 0.01           # the comparison is not one of zeros


def test_end_point_error_against_the_exact_flow():
    shape = SHAPES[2]
    n, tl, H, W = shape
    r32, r64 = _ref(shape, 'bumps', 0)
    batch = _input(shape, 'bumps')[1]
    flow = _run(shape, 'bumps', 0).cpu().numpy().astype(np.float64)
    for i, j in flow_ref.pairs(tl):
        truth = batch[f'flow_{i}{j}'][:, 0].astype(np.float64)
        epe = lambda f: float(np.sqrt(((f[:, i * tl + j] - truth) ** 2).sum(1)).mean())
        dev, ref = epe(flow), epe(r64['flow'])
        print(f'pair {i}{j}: mean end-point error device {dev:.5f} px, float64 restatement {ref:.5f} px, '
              f'mean true flow {np.sqrt((truth ** 2).sum(1)).mean():.3f} px')
        assert dev <= ref + flow_ref.stage_tolerance(r32['flow'], r64['flow'])
        assert ref < 0.5


def test_repeatable_and_independent_of_debug_outputs_workspace_and_layout():
    from depthinspace_amd import ops, lib
    shape = SHAPES[0]
    n, tl, H, W = shape
    a, dbg = _run(shape, 'bumps', 0, want_debug=True)
    b, dbg2 = _run(shape, 'bumps', 0, want_debug=True)
    c = _run(shape, 'bumps', 0)
    need = lib.fn('dis_flow_workspace')(n, tl, H, W, 8)
    ws = torch.full((need + 64,), 0xff, dtype=torch.uint8, device='cuda')
    d = _run(shape, 'bumps', 0, workspace=ws)
    e = ops.dense_flow(torch.from_numpy(_input(shape, 'bumps')[0]).cuda()[:, :, None], **PARAMS[0])   # (n, tl, 1, H, W)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(dbg['warp'], dbg2['warp'])
    assert all(torch.equal(x, y) for k in ('pyr', 'levels') for x, y in zip(dbg[k], dbg2[k]))
    assert torch.equal(a, c) and torch.equal(a, d)
    assert e.shape == a.shape and torch.equal(a, e)
    assert torch.equal(dbg['levels'][0].reshape(-1), a[:, [1, 2]].reshape(-1))   # tl = 2: entries 01 and 10


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[4]], ids=['2x3x24x40', '1x2x130x70'])
def test_one_launch_per_step_variant_gives_the_same_bits(shape):
    for pi in range(len(PARAMS)):
        a, b = _run(shape, 'bumps', pi), _run(shape, 'bumps', pi, variant=1)
        torch.cuda.synchronize()
        assert torch.equal(a, b), pi


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1]], ids=['1x2x37x83', '2x3x24x40'])
def test_graph_capture_on_a_side_stream(shape):
    from depthinspace_amd import ops, lib
    n, tl, H, W = shape
    fr = _input(shape, 'bumps')[0]
    eager = _run(shape, 'bumps', 0)
    fr_d = torch.zeros(shape, device='cuda')
    ws = torch.empty(lib.fn('dis_flow_workspace')(n, tl, H, W, 8), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.dense_flow(fr_d, workspace=ws, **PARAMS[0])
    fr_d.copy_(torch.from_numpy(fr))                 # the capture executed nothing: the replay sees the frames
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    ws.fill_(0xff)                                   # the workspace needs no initialisation and carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, eager) and torch.equal(out, eager)


def test_unsupported_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    ok = dict(n=1, tl=2, h=16, w=24, alpha=1.0, warps=3, iters=64, min_size=8)
    bad = [dict(tl=1), dict(tl=5), dict(h=7), dict(w=7), dict(h=8193), dict(w=8193), dict(alpha=0.0), dict(alpha=-1.0), dict(warps=0),
           dict(warps=17), dict(iters=0), dict(iters=1025), dict(min_size=3)]
    # 1. the wrapper: nothing is allocated or launched
    for kw in bad:
        a = dict(ok, **kw)
        fr = torch.zeros(a['n'], a['tl'], a['h'], a['w'], device='cuda')
        with pytest.raises(lib.DisHipError):
            ops.dense_flow(fr, alpha=a['alpha'], warps=a['warps'], iters=a['iters'], min_size=a['min_size'])
    fr = torch.zeros(1, 2, 16, 24, device='cuda')
    need = lib.fn('dis_flow_workspace')(1, 2, 16, 24, 8)
    ws = torch.empty(need + 16, dtype=torch.uint8, device='cuda')
    for w_ in (ws[:need - 1], ws[1:]):                # short; misaligned
        with pytest.raises(lib.DisHipError):
            ops.dense_flow(fr, workspace=w_)
    # 2. the entry point itself: a sentinel output stays untouched
    big = torch.zeros(5 * 8193 * 24, device='cuda')   # frames enough for every refused shape
    out = torch.full((25 * 2 * 8193 * 24,), -7.0, device='cuda')
    for kw in bad:
        a = dict(ok, **kw)
        with pytest.raises(lib.DisHipError):
            lib.call('dis_dense_flow', big, out, None, a['n'], a['tl'], a['h'], a['w'], a['alpha'], a['warps'], a['iters'], a['min_size'], ws)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_dense_flow', big, out, None, 1, 2, 16, 24, 1.0, 3, 64, 8, ws[1:])
    with pytest.raises(lib.DisHipError):
        lib.call('dis_dense_flow', big, out, None, 1, 2, 16, 24, 1.0, 3, 64, 8, None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    q = lib.fn('dis_flow_workspace')
    assert q(1, 2, 16, 24, 8) > 0
    for kw in bad:
        if not ({'alpha', 'warps', 'iters'} & set(kw)):
            a = dict(ok, **kw)
            assert q(a['n'], a['tl'], a['h'], a['w'], a['min_size']) == -1, kw
    assert q(0, 2, 16, 24, 8) == -1 and q(1 << 20, 4, 64, 64, 8) == -1
