"""GPU: dis_refine_track_poses (csrc/pose.hip) against the numpy restatement tests/pose_joint_ref.py, plus repeatability, full writes,
graph capture, the refusal of unsupported arguments, and dis_track_poses - whose per-pixel body the two accumulate kernels now share -
against its own restatement.

Nothing here is a stored number.  The restatement runs on the same input and the same starting point (tests/pose_joint_inputs.py: the
float64 pairwise restatement chained from frame 0, a fixed input that does not depend on the device) with float32 per-pixel terms and
float64 sums - what the kernels do - and in float64.  The counts, the contributing flags and the status must equal the float32
restatement exactly; the poses and the ratio statistics may deviate from the float64 values by pose_ref.tolerance = 16 max|ref32 - ref64|
+ 16 2^-23 max(1, max|ref64|).  tests/test_pose_joint_ref_cpu.py holds that the two restatements agree on the counts and that the
tolerance stays below 1e-4."""
import ctypes

import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import pose_inputs as PI
from tests import pose_joint_inputs as JI
from tests import pose_ref

pytestmark = pytest.mark.gpu

KEYS = ('R', 't', 'pair_stats', 'track_stats')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _run(shape, kind, pi=0, which='pairwise', masked=False, layout5=False, use=None, **kw):
    from depthinspace_amd import ops
    a = JI.make_input(shape, kind)
    R0, t0, status = JI.init(shape, kind, which)
    iters, scale, damping = JI.PARAMS[pi]
    disp = _dev(a['disp'])
    if layout5:
        disp = disp[:, :, None]
    if use is None and masked:
        use = status
    return ops.refine_track_poses(disp, _dev(a['flow']), a['K'], a['baseline'], _dev(R0), _dev(t0), None if use is None else _dev(use),
                                  iters=iters, scale=scale, damping=damping, min_corr=JI.MIN_CORR, **kw)


def _compare(got, r32, r64, shape, tag):
    n, tl, H, W = shape
    torch.cuda.synchronize()
    R, t, ps, ts = (_np(got[k]) for k in KEYS)
    assert R.shape == (n, tl, 3, 3) and t.shape == (n, tl, 3) and ps.shape == (n, tl, tl, 4) and ts.shape == (n, 4)
    assert all(x.dtype == np.float32 for x in (R, t, ps, ts))
    assert np.array_equal(ps[..., 0], r32['pair_stats'][..., 0]), 'the number of pixels used'
    assert np.array_equal(ps[..., 3], r32['pair_stats'][..., 3]), 'contributed'
    for k, name in ((0, 'contributing pairs'), (1, 'sum n'), (3, 'status')):
        assert np.array_equal(ts[..., k], r32['track_stats'][..., k]), name
    for name, g, a32, a64 in (('R', R, r32['R'], r64['R']), ('t', t, r32['t'], r64['t']),
                              ('mean weight', ps[..., 1], r32['pair_stats'][..., 1], r64['pair_stats'][..., 1]),
                              ('rms residual', ps[..., 2], r32['pair_stats'][..., 2], r64['pair_stats'][..., 2]),
                              ('track rms residual', ts[..., 2], r32['track_stats'][..., 2], r64['track_stats'][..., 2])):
        allowed = pose_ref.tolerance(a32, a64)
        err = float(np.abs(g.astype(np.float64) - a64).max())
        print(f'{tag} {name}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}, max |device - ref32| '
              f'{float(np.abs(g.astype(np.float64) - a32.astype(np.float64)).max()):.3e}')
        assert np.isfinite(g).all() and err <= allowed, (name, err, allowed)
    return R, t, ps, ts


@pytest.mark.parametrize('case', JI.CASES, ids=JI.case_id)
def test_against_the_restatement(case):
    shape, kind = case
    r32, r64 = JI.refs(shape, kind, 0)
    R, t, ps, ts = _compare(_run(shape, kind), r32, r64, shape, 'params 0')
    R0, t0, _ = JI.init(shape, kind)
    if JI.base_kind(kind) != 'no_overlap' and shape != JI.SHAPES[0]:
        assert np.all(ts[:, 3] == 1)
        if JI.base_kind(kind) not in ('plane', 'holes') or kind != JI.base_kind(kind):      # the comparison is not one of copies of the init
            assert not np.array_equal(R, R0)
    else:
        assert np.all(ts[:, 3] == 0) and np.array_equal(R, R0) and np.array_equal(t, t0)


@pytest.mark.parametrize('pi', [1, 2])
@pytest.mark.parametrize('case', [(JI.SHAPES[2], 'noise'), (JI.SHAPES[3], 'contam+broken')], ids=JI.case_id)
def test_against_the_restatement_at_other_parameters(case, pi):
    shape, kind = case
    _compare(_run(shape, kind, pi), *JI.refs(shape, kind, pi), shape, f'params {pi}')


@pytest.mark.parametrize('case', [(JI.SHAPES[3], 'render'), (JI.SHAPES[2], 'bumps')], ids=JI.case_id)
def test_from_the_perturbed_truth(case):
    shape, kind = case
    _compare(_run(shape, kind, which='perturbed'), *JI.refs(shape, kind, 0, 'perturbed'), shape, 'perturbed')


def _use_without_frame_2(shape):
    n, tl = shape[:2]
    use = np.ones((n, tl, tl), np.uint8)
    use[:, 2, :] = 0
    use[:, :, 2] = 0
    return use


def test_masked_pairs():
    """pair_use = the pairwise status (every pair at 64 x 96 noise+broken, none at no_overlap), and a mask that leaves frame 2 without a
    pair: the track fails and keeps the init"""
    from tests import pose_joint_ref
    shape = JI.SHAPES[3]
    _compare(_run(shape, 'noise+broken', masked=True), *JI.refs(shape, 'noise+broken', 0, masked=True), shape, 'status mask')
    got = _run(shape, 'no_overlap', masked=True)
    _compare(got, *JI.refs(shape, 'no_overlap', 0, masked=True), shape, 'empty mask')
    assert bool((got['track_stats'] == 0).all())
    use = _use_without_frame_2(shape)
    a = JI.make_input(shape, 'noise')
    R0, t0, _ = JI.init(shape, 'noise')
    iters, scale, damping = JI.PARAMS[0]
    refs = [pose_joint_ref.refine_track_poses(a['disp'], a['flow'], a['K'], a['baseline'], R0, t0, use, iters, scale, damping, JI.MIN_CORR,
                                              dtype=dt) for dt in (np.float32, np.float64)]
    got = _run(shape, 'noise', use=use)
    R, t, ps, ts = _compare(got, *refs, shape, 'frame 2 untouched')
    assert ts[0, 3] == 0 and ts[0, 0] == 6 and np.array_equal(R, R0) and np.array_equal(t, t0)
    assert np.all(ps[0, 2, [0, 1, 3]] == 0) and np.all(ps[0, [0, 1, 3], 2] == 0)
    # the flows of the pairs that are not used are not read into the result
    flow = a['flow'].copy()
    for i in range(4):
        for j in range(4):
            if i != j and not use[0, i, j]:
                flow[:, i * 4 + j] = np.nan
    from depthinspace_amd import ops
    other = ops.refine_track_poses(_dev(a['disp']), _dev(flow), a['K'], a['baseline'], _dev(R0), _dev(t0), _dev(use), min_corr=JI.MIN_CORR)
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), other[k].view(torch.int32)), k
    # a bool mask is the same mask
    other = _run(shape, 'noise', use=use.astype(bool))
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), other[k].view(torch.int32)), k


def test_repeatable_and_independent_of_workspace_and_layout():
    from depthinspace_amd import lib, ops
    shape = JI.SHAPES[3]
    n, tl, H, W = shape
    a = _run(shape, 'noise+broken')
    b = _run(shape, 'noise+broken')
    ws = torch.full((lib.fn('dis_pose_joint_workspace')(n, tl, H, W) + 64,), 0xff, dtype=torch.uint8, device='cuda')
    c = _run(shape, 'noise+broken', workspace=ws)
    d = _run(shape, 'noise+broken', layout5=True)
    torch.cuda.synchronize()
    assert bool((a['track_stats'][:, 3] == 1).all())
    for other in (b, c, d):
        for k in KEYS:
            assert torch.equal(a[k].view(torch.int32), other[k].view(torch.int32)), k
    # a track's result does not depend on what else is in the call
    two = JI.SHAPES[2]
    x = JI.make_input(two, 'bumps')
    R0, t0, _ = JI.init(two, 'bumps')
    both = _run(two, 'bumps')
    for b_ in range(two[0]):
        s = slice(b_, b_ + 1)
        one = ops.refine_track_poses(_dev(x['disp'][s]), _dev(x['flow'][s]), x['K'], x['baseline'], _dev(R0[s]), _dev(t0[s]),
                                     min_corr=JI.MIN_CORR)
        for k in KEYS:
            assert torch.equal(one[k][0].view(torch.int32), both[k][b_].view(torch.int32)), (b_, k)


def _raw(lib, disp, flow, K4, baseline, R0, t0, use, iters, scale, damping, min_corr, R, t, ps, ts, n, tl, h, w, ws, nbytes):
    """the entry point itself -> its return code"""
    p = lambda x: None if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else ctypes.cast(x, ctypes.c_void_p))
    return lib.fn('dis_refine_track_poses')(p(disp), p(flow), p(K4), baseline, p(R0), p(t0), p(use), iters, scale, damping, min_corr, p(R),
                                            p(t), p(ps), p(ts), n, tl, h, w, p(ws), nbytes, torch.cuda.current_stream().cuda_stream)


def _sizes(n, tl):
    return (n * tl * 9, n * tl * 3, n * tl * tl * 4, n * 4)


@pytest.mark.parametrize('case', [(JI.SHAPES[0], 'plane', None), (JI.SHAPES[2], 'holes', None), (JI.SHAPES[3], 'no_overlap', None),
                                  (JI.SHAPES[3], 'noise', 'frame2'), (JI.SHAPES[3], 'noise+broken', 'status')],
                         ids=lambda c: f'{JI.case_id(c[:2])}-{c[2]}')
def test_every_output_element_is_written(case):
    from depthinspace_amd import lib
    shape, kind, mask = case
    n, tl, H, W = shape
    a = JI.make_input(shape, kind)
    R0, t0, status = JI.init(shape, kind)
    use = None if mask is None else (status if mask == 'status' else _use_without_frame_2(shape))
    pad = 16
    outs = [torch.full((m + pad,), float('nan'), device='cuda') for m in _sizes(n, tl)]
    need = lib.fn('dis_pose_joint_workspace')(n, tl, H, W)
    ws = torch.full((need,), 0xff, dtype=torch.uint8, device='cuda')
    K4 = lib.host_floats([a['K'][0, 0], a['K'][1, 1], a['K'][0, 2], a['K'][1, 2]])
    rc = _raw(lib, _dev(a['disp']), _dev(a['flow']), K4, a['baseline'], _dev(R0), _dev(t0), None if use is None else _dev(use), 6, 1.0, 0.0,
              JI.MIN_CORR, *outs, n, tl, H, W, ws, need)
    torch.cuda.synchronize()
    assert rc == 0
    want = _run(shape, kind, use=use)
    for o, k, used in zip(outs, KEYS, _sizes(n, tl)):
        assert not bool(torch.isnan(o[:used]).any()) and bool(torch.isnan(o[used:]).all()), k     # all of it, and nothing past it
        assert torch.equal(o[:used].view(torch.int32), want[k].reshape(-1).view(torch.int32)), k
    eye = torch.eye(tl, dtype=torch.bool, device='cuda')
    assert bool((want['pair_stats'][:, eye] == torch.tensor([0.0, 0.0, 0.0, 1.0], device='cuda')).all())
    # frame 0 is never moved
    assert torch.equal(want['R'][:, 0].view(torch.int32), _dev(R0)[:, 0].view(torch.int32))
    assert torch.equal(want['t'][:, 0].view(torch.int32), _dev(t0)[:, 0].view(torch.int32))


def test_frame_0_keeps_its_bits_when_it_is_not_the_identity():
    shape = JI.SHAPES[3]
    R0, t0, _ = JI.init(shape, 'render', 'perturbed')
    assert not np.array_equal(R0[:, 0], np.broadcast_to(np.eye(3, dtype=np.float32), R0[:, 0].shape)) or np.any(t0[:, 0] != 0)
    got = _run(shape, 'render', which='perturbed')
    assert np.array_equal(_np(got['R'])[:, 0].view(np.int32), R0[:, 0].view(np.int32))
    assert np.array_equal(_np(got['t'])[:, 0].view(np.int32), t0[:, 0].view(np.int32))
    assert bool((got['track_stats'][:, 3] == 1).all()) and not np.array_equal(_np(got['R'])[:, 1:], R0[:, 1:])


@pytest.mark.parametrize('shape', [JI.SHAPES[1], JI.SHAPES[2]], ids=PI.shape_id)
def test_graph_capture_on_a_side_stream(shape):
    from depthinspace_amd import ops, lib
    n, tl, H, W = shape
    a = JI.make_input(shape, 'bumps')
    R0, t0, _ = JI.init(shape, 'bumps')
    eager = _run(shape, 'bumps')
    disp_d, flow_d = torch.zeros(shape, device='cuda'), torch.zeros(a['flow'].shape, device='cuda')
    R_d, t_d = torch.zeros(R0.shape, device='cuda'), torch.zeros(t0.shape, device='cuda')
    ws = torch.empty(lib.fn('dis_pose_joint_workspace')(n, tl, H, W), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.refine_track_poses(disp_d, flow_d, a['K'], a['baseline'], R_d, t_d, min_corr=JI.MIN_CORR, workspace=ws)
    disp_d.copy_(_dev(a['disp']))                    # the capture executed nothing: the replay sees the inputs
    flow_d.copy_(_dev(a['flow']))
    R_d.copy_(_dev(R0))
    t_d.copy_(_dev(t0))
    ws.fill_(0xff)                                   # the workspace needs no initialisation
    graph.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)), k


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
    poses = lambda n, tl: (torch.eye(3, device='cuda').expand(n, tl, 3, 3).contiguous(), torch.zeros(n, tl, 3, device='cuda'))
    # 1. the wrapper: nothing is allocated or launched
    for kw in shapes[:-1] + params:
        a = dict(ok, **kw)
        disp = torch.ones(a['n'], a['tl'], a['h'], a['w'], device='cuda')
        flow = torch.zeros(a['n'], a['tl'] * a['tl'], 2, a['h'], a['w'], device='cuda')
        with pytest.raises(lib.DisHipError):
            ops.refine_track_poses(disp, flow, K(a), a['baseline'], *poses(a['n'], a['tl']), iters=a['iters'], scale=a['scale'],
                                   damping=a['damping'], min_corr=a['min_corr'])
    disp, flow = torch.ones(1, 2, 16, 24, device='cuda'), torch.zeros(1, 4, 2, 16, 24, device='cuda')
    R0, t0 = poses(1, 2)
    need = lib.fn('dis_pose_joint_workspace')(1, 2, 16, 24)
    ws = torch.empty(need + 16, dtype=torch.uint8, device='cuda')
    for w_ in (ws[:need - 1], ws[1:]):                # short; misaligned
        with pytest.raises(lib.DisHipError):
            ops.refine_track_poses(disp, flow, K(ok), 0.05, R0, t0, workspace=w_)
    with pytest.raises(RuntimeError):
        ops.refine_track_poses(disp, flow, K(ok), 0.05, R0, t0, workspace=ws.cpu())
    # CPU tensors and wrong layouts: the HIP path is the only path
    use = torch.ones(1, 2, 2, dtype=torch.uint8, device='cuda')
    for d_, f_, R_, t_, u_ in ((disp.cpu(), flow, R0, t0, None), (disp, flow.cpu(), R0, t0, None), (disp, flow, R0.cpu(), t0, None),
                               (disp, flow, R0, t0.cpu(), None), (disp, flow, R0, t0, use.cpu()), (disp.double(), flow, R0, t0, None),
                               (disp, flow, R0.double(), t0, None), (disp, flow, R0, t0, use.float()), (disp, flow, R0, t0, use.int()),
                               (disp, flow[:, :3], R0, t0, None), (disp, flow, R0[:, :1], t0, None), (disp, flow, R0, t0[:, :1], None),
                               (disp, flow, R0.view(1, 2, 9), t0, None), (disp, flow, R0, t0, use.view(1, 4)),
                               (disp, flow, R0, t0, use.expand(1, 2, 2, 2)[..., 0]), (disp[0], flow[0], R0, t0, None)):
        with pytest.raises(RuntimeError):
            ops.refine_track_poses(d_, f_, K(ok), 0.05, R_, t_, u_)
    # 2. the entry point itself: codes and their order; NaN-filled outputs stay untouched
    big = torch.ones(5 * 8193 * 24, device='cuda')    # disparities, flows and poses enough for every refused shape that could launch
    outs = [torch.full((m,), nan, device='cuda') for m in _sizes(5, 5)]
    wsb = torch.empty(lib.fn('dis_pose_joint_workspace')(1, 4, 8192, 24) + 16, dtype=torch.uint8, device='cuda')

    def raw(a, disp=big, flow=big, K4=True, R0=big, t0=big, use=None, outs=outs, workspace=wsb, nbytes=None):
        K4 = lib.host_floats([a['fx'], a['fy'], a['cx'], a['cy']]) if K4 else None
        return _raw(lib, disp, flow, K4, a['baseline'], R0, t0, use, a['iters'], a['scale'], a['damping'], a['min_corr'], *outs, a['n'],
                    a['tl'], a['h'], a['w'], workspace, workspace.numel() if nbytes is None and workspace is not None else (nbytes or 0))

    for kw in shapes:
        assert raw(dict(ok, **kw)) == BAD_SHAPE, kw
    for kw in params:
        assert raw(dict(ok, **kw)) == UNSUPPORTED, kw
    assert raw(ok, workspace=wsb[1:], nbytes=wsb.numel() - 1) == UNSUPPORTED          # misaligned
    assert raw(ok, nbytes=need - 1) == UNSUPPORTED                                    # short
    worst = dict(ok, n=0, iters=0, fx=nan)
    assert raw(worst, disp=None) == NULL and raw(worst, flow=None) == NULL and raw(worst, K4=False) == NULL and raw(worst, workspace=None) == NULL
    assert raw(worst, R0=None) == NULL and raw(worst, t0=None) == NULL
    for k in range(4):
        assert raw(worst, outs=[None if m == k else o for m, o in enumerate(outs)]) == NULL
    assert raw(worst) == BAD_SHAPE and raw(dict(ok, tl=5, scale=-1.0), nbytes=0) == BAD_SHAPE   # the shape comes before the parameters
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    assert raw(ok, R0=R0, t0=t0) == 0                  # the same call with nothing wrong goes through, pair_use NULL
    torch.cuda.synchronize()
    for o, m in zip(outs, _sizes(1, 2)):
        assert not bool(torch.isnan(o[:m]).any()) and bool(torch.isnan(o[m:]).all())
    q = lib.fn('dis_pose_joint_workspace')
    assert q(1, 2, 16, 24) > 0 and q(1, 2, 2, 2) > 0 and q(1, 2, 8192, 8192) > 0 and q(1, 4, 8192, 8192) == -1
    for kw in shapes:
        a = dict(ok, **kw)
        assert q(a['n'], a['tl'], a['h'], a['w']) == -1, kw
    assert q(1 << 20, 4, 64, 64) == -1 and q(4, 4, 8192, 8192) == -1 and q(-1, 2, 16, 24) == -1


@pytest.mark.parametrize('case', [(PI.SHAPES[3], 'noise'), (PI.SHAPES[2], 'holes')], ids=PI.case_id)
def test_the_pairwise_estimate_is_what_it_was(case):
    """dis_track_poses runs the per-pixel function it now shares with the joint kernel: against its float32 restatement, as
    tests/test_pose_gpu.py compares it (that file, unchanged, is the full check)"""
    from depthinspace_amd import ops
    shape, kind = case
    a = PI.make_input(shape, kind)
    iters, scale, damping = PI.PARAMS[0]
    r32, r64 = PI.refs(shape, kind, 0)
    got = ops.track_poses(_dev(a['disp']), _dev(a['flow']), a['K'], a['baseline'], iters=iters, scale=scale, damping=damping,
                          min_corr=PI.MIN_CORR)
    torch.cuda.synchronize()
    R, t, st = (_np(got[k]) for k in ('R_pair', 't_pair', 'stats'))
    assert np.array_equal(st[..., 0], r32['stats'][..., 0]) and np.array_equal(st[..., 3], r32['stats'][..., 3])
    for name, g, a32, a64 in (('R_pair', R, r32['R_pair'], r64['R_pair']), ('t_pair', t, r32['t_pair'], r64['t_pair']),
                              ('mean weight', st[..., 1], r32['stats'][..., 1], r64['stats'][..., 1]),
                              ('rms residual', st[..., 2], r32['stats'][..., 2], r64['stats'][..., 2])):
        allowed = pose_ref.tolerance(a32, a64)
        err = float(np.abs(g.astype(np.float64) - a64).max())
        print(f'{name}: max |device - ref64| {err:.3e}, allowed {allowed:.3e}')
        assert np.isfinite(g).all() and err <= allowed, (name, err, allowed)
