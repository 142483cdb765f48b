"""GPU: dis_track_poses (csrc/pose.hip) against the numpy restatement tests/pose_ref.py, plus repeatability, full writes, graph capture
and the refusal of unsupported arguments.

Nothing here is a stored number.  The restatement runs on the same input with float32 per-pixel terms and float64 sums - what the
kernels do - and in float64.  The counts and the status must equal the float32 restatement exactly; the poses and the two ratio
statistics may deviate from the float64 values by pose_ref.tolerance = 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|).
tests/test_pose_ref_cpu.py holds, for every case, that the two restatements agree on the counts and that the tolerance stays below 1e-4."""
import ctypes

import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import pose_inputs as PI
from tests import pose_ref

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(shape, kind, pi=0, layout5=False, **kw):
    from depthinspace_amd import ops
    a = PI.make_input(shape, kind)
    iters, scale, damping = PI.PARAMS[pi]
    disp = _dev(a['disp'])
    if layout5:
        disp = disp[:, :, None]
    return ops.track_poses(disp, _dev(a['flow']), a['K'], a['baseline'], iters=iters, scale=scale, damping=damping, min_corr=PI.MIN_CORR, **kw)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('case', PI.CASES, ids=PI.case_id)
def test_against_the_restatement(case):
    shape, kind = case
    n, tl, H, W = shape
    for pi in range(len(PI.PARAMS)):
        r32, r64 = PI.refs(shape, kind, pi)
        got = _run(shape, kind, pi)
        torch.cuda.synchronize()
        R, t, st = (_np(got[k]) for k in ('R_pair', 't_pair', 'stats'))
        assert R.shape == (n, tl, tl, 3, 3) and t.shape == (n, tl, tl, 3) and st.shape == (n, tl, tl, 4)
        assert all(x.dtype == np.float32 for x in (R, t, st))
        assert np.array_equal(st[..., 0], r32['stats'][..., 0]), 'the number of pixels used'
        assert np.array_equal(st[..., 3], r32['stats'][..., 3]), 'status'
        for name, g, a32, a64 in (('R_pair', R, r32['R_pair'], r64['R_pair']), ('t_pair', t, r32['t_pair'], r64['t_pair']),
                                  ('mean weight', st[..., 1], r32['stats'][..., 1], r64['stats'][..., 1]),
                                  ('rms residual', st[..., 2], r32['stats'][..., 2], r64['stats'][..., 2])):
            allowed = pose_ref.tolerance(a32, a64)
            err = float(np.abs(g.astype(np.float64) - a64).max())
            print(f'params {pi} {name}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, max |device - ref32| '
                  f'{float(np.abs(g.astype(np.float64) - a32.astype(np.float64)).max()):.3e}')
            assert np.isfinite(g).all() and err <= allowed, (name, err, allowed)
    # the comparison is not one of identities
    if kind not in ('no_overlap',) and H * W > 4:
        assert bool((got['stats'][..., 3] == 1).all()) and float(np.abs(R - np.eye(3, dtype=np.float32)).max()) > 1e-4


def test_repeatable_and_independent_of_workspace_and_layout():
    from depthinspace_amd import lib
    shape = PI.SHAPES[3]
    n, tl, H, W = shape
    a = _run(shape, 'noise')
    b = _run(shape, 'noise')
    ws = torch.full((lib.fn('dis_pose_workspace')(n, tl, H, W) + 64,), 0xff, dtype=torch.uint8, device='cuda')
    c = _run(shape, 'noise', workspace=ws)
    d = _run(shape, 'noise', layout5=True)
    torch.cuda.synchronize()
    assert bool((a['stats'][..., 3] == 1).all())
    for other in (b, c, d):
        for k in a:
            assert torch.equal(a[k].view(torch.int32), other[k].view(torch.int32)), k
    # a track's result does not depend on what else is in the call
    two = PI.SHAPES[2]
    x = PI.make_input(two, 'bumps')
    both = _run(two, 'bumps')
    from depthinspace_amd import ops
    for b_ in range(two[0]):
        one = ops.track_poses(_dev(x['disp'][b_:b_ + 1]), _dev(x['flow'][b_:b_ + 1]), x['K'], x['baseline'], min_corr=PI.MIN_CORR)
        for k in one:
            assert torch.equal(one[k][0].view(torch.int32), both[k][b_].view(torch.int32)), (b_, k)


def _raw(lib, disp, flow, K4, baseline, iters, scale, damping, min_corr, R, t, st, n, tl, h, w, ws, nbytes):
    """the entry point itself -> its return code"""
    p = lambda x: None if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else ctypes.cast(x, ctypes.c_void_p))
    return lib.fn('dis_track_poses')(p(disp), p(flow), p(K4), baseline, iters, scale, damping, min_corr, p(R), p(t), p(st), n, tl, h, w,
                                     p(ws), nbytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('case', [(PI.SHAPES[0], 'plane'), (PI.SHAPES[2], 'holes'), (PI.SHAPES[3], 'no_overlap')], ids=PI.case_id)
def test_every_output_element_is_written(case):
    from depthinspace_amd import lib
    shape, kind = case
    n, tl, H, W = shape
    a = PI.make_input(shape, kind)
    pad = 16
    outs = [torch.full((n * tl * tl * m + pad,), float('nan'), device='cuda') for m in (9, 3, 4)]
    need = lib.fn('dis_pose_workspace')(n, tl, H, W)
    ws = torch.full((need,), 0xff, dtype=torch.uint8, device='cuda')
    K4 = lib.host_floats([a['K'][0, 0], a['K'][1, 1], a['K'][0, 2], a['K'][1, 2]])
    rc = _raw(lib, _dev(a['disp']), _dev(a['flow']), K4, a['baseline'], 6, 1.0, 0.0, PI.MIN_CORR, *outs, n, tl, H, W, ws, need)
    torch.cuda.synchronize()
    assert rc == 0
    want = _run(shape, kind)
    for o, k, m in zip(outs, ('R_pair', 't_pair', 'stats'), (9, 3, 4)):
        used = n * tl * tl * m
        assert not bool(torch.isnan(o[:used]).any()) and bool(torch.isnan(o[used:]).all()), k     # all of it, and nothing past it
        assert torch.equal(o[:used].view(torch.int32), want[k].reshape(-1).view(torch.int32)), k
    eye = torch.eye(tl, dtype=torch.bool, device='cuda')
    assert bool((want['R_pair'][:, eye] == torch.eye(3, device='cuda')).all()) and bool((want['t_pair'][:, eye] == 0).all())
    assert bool((want['stats'][:, eye] == torch.tensor([0.0, 0.0, 0.0, 1.0], device='cuda')).all())


@pytest.mark.parametrize('shape', [PI.SHAPES[1], PI.SHAPES[2]], ids=PI.shape_id)
def test_graph_capture_on_a_side_stream(shape):
    from depthinspace_amd import ops, lib
    n, tl, H, W = shape
    a = PI.make_input(shape, 'bumps')
    eager = _run(shape, 'bumps')
    disp_d, flow_d = torch.zeros(shape, device='cuda'), torch.zeros(a['flow'].shape, device='cuda')
    ws = torch.empty(lib.fn('dis_pose_workspace')(n, tl, H, W), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.track_poses(disp_d, flow_d, a['K'], a['baseline'], min_corr=PI.MIN_CORR, workspace=ws)
    disp_d.copy_(_dev(a['disp']))                    # the capture executed nothing: the replay sees the inputs
    flow_d.copy_(_dev(a['flow']))
    graph.replay()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    ws.fill_(0xff)                                   # the workspace needs no initialisation and carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    for res in (first, out):
        for k in eager:
            assert torch.equal(res[k].view(torch.int32), eager[k].view(torch.int32)), k


def test_unsupported_arguments_are_refused_in_the_documented_order():
    from depthinspace_amd import ops, lib
    NULL, BAD_SHAPE, UNSUPPORTED = -3, -1, -2
    inf, nan = float('inf'), float('nan')
    ok = dict(n=1, tl=2, h=16, w=24, iters=6, scale=1.0, damping=0.0, min_corr=64, fx=100.0, fy=100.0, cx=10.0, cy=8.0, baseline=0.05)
    shapes = [dict(n=0), dict(tl=1), dict(tl=5), dict(h=1), dict(w=1), dict(h=8193), dict(w=8193), dict(n=1400, tl=4, h=256, w=256)]
    params = [dict(iters=0), dict(iters=65), dict(scale=0.0), dict(scale=-1.0), dict(scale=inf), dict(scale=nan), dict(damping=-1e-3),
              dict(damping=inf), dict(damping=nan), dict(min_corr=5), dict(fx=0.0), dict(fx=-1.0), dict(fx=inf), dict(fx=nan), dict(fy=0.0),
              dict(fy=inf), dict(fy=nan), dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=inf), dict(baseline=nan), dict(cx=inf),
              dict(cx=nan), dict(cy=-inf), dict(cy=nan)]
    K = lambda a: np.array([[a['fx'], 0, a['cx']], [0, a['fy'], a['cy']], [0, 0, 1]], dtype=np.float64)
    # 1. the wrapper: nothing is allocated or launched
    for kw in shapes[:-1] + params:
        a = dict(ok, **kw)
        disp = torch.ones(a['n'], a['tl'], a['h'], a['w'], device='cuda')
        flow = torch.zeros(a['n'], a['tl'] * a['tl'], 2, a['h'], a['w'], device='cuda')
        with pytest.raises(lib.DisHipError):
            ops.track_poses(disp, flow, K(a), a['baseline'], iters=a['iters'], scale=a['scale'], damping=a['damping'], min_corr=a['min_corr'])
    disp, flow = torch.ones(1, 2, 16, 24, device='cuda'), torch.zeros(1, 4, 2, 16, 24, device='cuda')
    need = lib.fn('dis_pose_workspace')(1, 2, 16, 24)
    ws = torch.empty(need + 16, dtype=torch.uint8, device='cuda')
    for w_ in (ws[:need - 1], ws[1:]):                # short; misaligned
        with pytest.raises(lib.DisHipError):
            ops.track_poses(disp, flow, K(ok), 0.05, workspace=w_)
    with pytest.raises(RuntimeError):
        ops.track_poses(disp, flow, K(ok), 0.05, workspace=ws.cpu())
    # CPU tensors and wrong layouts: the HIP path is the only path
    for d_, f_ in ((disp.cpu(), flow), (disp, flow.cpu()), (disp.double(), flow), (disp, flow.half()), (disp[..., ::2], flow[..., ::2]),
                   (disp.transpose(2, 3), flow.transpose(3, 4)), (disp, flow[:, :3]), (disp, flow.view(1, 2, 4, 16, 24)),
                   (disp[0], flow[0]), (disp.view(1, 2, 1, 1, 16, 24), flow), (disp.view(1, 1, 2, 16, 24), flow)):
        with pytest.raises(RuntimeError):
            ops.track_poses(d_, f_, K(ok), 0.05)
    # 2. the entry point itself: codes and their order; NaN-filled outputs stay untouched
    big = torch.ones(5 * 8193 * 24, device='cuda')    # disparities and flows enough for every refused shape that could launch
    outs = [torch.full((5 * 16 * m,), nan, device='cuda') for m in (9, 3, 4)]
    wsb = torch.empty(lib.fn('dis_pose_workspace')(1, 4, 8192, 24) + 16, dtype=torch.uint8, device='cuda')

    def raw(a, disp=big, flow=big, K4=True, outs=outs, workspace=wsb, nbytes=None):
        K4 = lib.host_floats([a['fx'], a['fy'], a['cx'], a['cy']]) if K4 else None
        return _raw(lib, disp, flow, K4, a['baseline'], a['iters'], a['scale'], a['damping'], a['min_corr'], *outs, a['n'], a['tl'], a['h'],
                    a['w'], workspace, workspace.numel() if nbytes is None and workspace is not None else (nbytes or 0))

    for kw in shapes:
        assert raw(dict(ok, **kw)) == BAD_SHAPE, kw
    for kw in params:
        assert raw(dict(ok, **kw)) == UNSUPPORTED, kw
    assert raw(ok, workspace=wsb[1:], nbytes=wsb.numel() - 1) == UNSUPPORTED          # misaligned
    assert raw(ok, nbytes=need - 1) == UNSUPPORTED                                    # short
    worst = dict(ok, n=0, iters=0, fx=nan)
    assert raw(worst, disp=None) == NULL and raw(worst, flow=None) == NULL and raw(worst, K4=False) == NULL and raw(worst, workspace=None) == NULL
    for k in range(3):
        assert raw(worst, outs=[None if m == k else o for m, o in enumerate(outs)]) == NULL
    assert raw(worst) == BAD_SHAPE and raw(dict(ok, tl=5, scale=-1.0), nbytes=0) == BAD_SHAPE   # the shape comes before the parameters
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    assert raw(ok) == 0                                # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    for o, m in zip(outs, (9, 3, 4)):
        assert not bool(torch.isnan(o[:4 * m]).any()) and bool(torch.isnan(o[4 * m:]).all())
    q = lib.fn('dis_pose_workspace')
    assert q(1, 2, 16, 24) > 0 and q(1, 2, 2, 2) > 0 and q(1, 2, 8192, 8192) > 0 and q(1, 4, 8192, 8192) == -1
    for kw in shapes:
        a = dict(ok, **kw)
        assert q(a['n'], a['tl'], a['h'], a['w']) == -1, kw
    assert q(1 << 20, 4, 64, 64) == -1 and q(4, 4, 8192, 8192) == -1 and q(-1, 2, 16, 24) == -1
