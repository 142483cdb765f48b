"""CPU: the numpy restatement of the pairwise pose estimation (tests/pose_ref.py) against the truth of its synthetic inputs - what the
GPU test (tests/test_pose_gpu.py) then holds the kernels to - and the parts of data/presave_pose.py and data/convert.py that need no
device.

Nothing here is a stored number: errors are measured against the poses the inputs were made with, and bounds come from the distance
between the float32 and the float64 restatement (pose_ref.tolerance) or from another estimate of the same quantity."""
import os

import numpy as np
import pytest

from tests import pose_inputs as PI
from tests import pose_ref

SMALLEST = PI.SHAPES[0]                      # every pair has fewer than MIN_CORR pixels
FITTED = [s for s in PI.SHAPES if s != SMALLEST]


def _offdiag(tl):
    return ~np.eye(tl, dtype=bool)


@pytest.mark.parametrize('shape', FITTED, ids=PI.shape_id)
def test_exact_planes_give_the_true_relative_poses(shape):
    a = PI.make_input(shape, 'plane')
    for pi in (0, 2):
        r32, r64 = PI.refs(shape, 'plane', pi)
        assert np.all(r64['stats'][..., 3] == 1) and np.all(r64['steps'][:, _offdiag(shape[1])] == PI.PARAMS[pi][0])
        for k in ('R_pair', 't_pair'):
            err, allowed = float(np.abs(r64[k] - a[k]).max()), pose_ref.tolerance(r32[k], r64[k])
            print(f'params {pi} {k}: max |ref64 - truth| {err:.3e}, allowed {allowed:.3e}')
            assert err <= allowed


@pytest.mark.parametrize('kind', ['plane', 'bumps', 'noise'])
@pytest.mark.parametrize('shape', FITTED, ids=PI.shape_id)
def test_the_objective_does_not_increase_after_the_first_step(shape, kind):
    """the objective of passes 1 .. iters (sum r2 g; pass 0 has another one, the unweighted sum r2).  At a converged state it is
    stationary and only its rounding moves it: a residual e formed from pixel coordinates up to max(H, W) carries an absolute error
    delta <= 16 2^-52 max(H, W), r2 = |e|^2 then 2 |e| delta + delta^2, and the sum over n pixels at most 2 sqrt(n cost) delta + n delta^2
    (Cauchy-Schwarz).  That much increase is allowed, no more."""
    n_, tl, H, W = shape
    delta = 16 * 2.0 ** -52 * max(H, W)
    for pi in range(len(PI.PARAMS)):
        r64 = PI.refs(shape, kind, pi)[1]
        cost, n = r64['cost'][:, _offdiag(tl)], r64['n_used'][:, _offdiag(tl)]
        assert np.all(n[..., 0] >= PI.MIN_CORR) and np.all(cost[..., 0] > 0)
        before, after = cost[..., 1:-1], cost[..., 2:]
        slack = 2 * np.sqrt(n[..., 1:-1] * before) * delta + n[..., 1:-1] * delta ** 2
        print(f'params {pi}: objective of pair (0, 1) {cost[0, 0]}, largest increase {float((after - before).max()) if after.size else 0:.3e}')
        assert np.all(after <= before + slack)
        assert np.all(cost[..., 1] < cost[..., 0])            # and the unweighted step itself gets closer


@pytest.mark.parametrize('shape', [PI.SHAPES[3], PI.SHAPES[4]], ids=PI.shape_id)
def test_the_redescending_weight_rejects_a_moving_region(shape):
    a = PI.make_input(shape, 'contam')
    iters, scale, damping = PI.PARAMS[0]
    assert iters == 6
    r6 = PI.refs(shape, 'contam', 0)[1]
    r1 = pose_ref.track_poses(a['disp'], a['flow'], a['K'], a['baseline'], 1, scale, damping, PI.MIN_CORR, dtype=np.float64)
    e6, e1 = PI.pose_error(r6, a), PI.pose_error(r1, a)
    print(f'max error of R, t after the unweighted step {e1[0]:.3e} {e1[1]:.3e}, after 6 steps {e6[0]:.3e} {e6[1]:.3e}')
    assert e6[0] < e1[0] and e6[1] < e1[1]


def _horn(di, dj, fl, K, baseline):
    """the closed-form rigid alignment (Horn / Kabsch) of the lifted points of the matched pixels, float64 -> R, t"""
    f = np.float64
    fx, fy, cx, cy = f(K[0, 0]), f(K[1, 1]), f(K[0, 2]), f(K[1, 2])
    fb = fx * f(baseline)
    P, uj, vj, ds = pose_ref._targets(di, dj, fl, fx, fy, cx, cy, fb, f)
    P = np.stack(P, 1)
    zq = fb / ds
    Q = np.stack([zq * ((uj - cx) / fx), zq * ((vj - cy) / fy), zq], 1)
    cp, cq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - cp).T @ (Q - cq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cq - R @ cp


@pytest.mark.parametrize('shape', FITTED, ids=PI.shape_id)
def test_on_noisy_input_it_is_closer_than_the_closed_form_alignment(shape):
    """the design choice: at this geometry 0.05 px of disparity noise is more than 1 % of the depth, which dominates a residual in 3D;
    the residual in (u, v, disparity) weighs the noise as it is.  On exact input the closed form is exact as well."""
    n, tl, H, W = shape
    for kind in ('noise', 'plane'):
        a = PI.make_input(shape, kind)
        Rh, th = np.zeros((n, tl, tl, 3, 3)), np.zeros((n, tl, tl, 3))
        for b in range(n):
            for i in range(tl):
                for j in range(tl):
                    Rh[b, i, j], th[b, i, j] = (np.eye(3), np.zeros(3)) if i == j else _horn(
                        a['disp'][b, i], a['disp'][b, j], a['flow'][b, i * tl + j], a['K'], a['baseline'])
        eh = PI.pose_error({'R_pair': Rh, 't_pair': th}, a)
        eg = PI.pose_error(PI.refs(shape, kind, 0)[1], a)
        print(f'{kind}: max error of R, t: closed form {eh[0]:.3e} {eh[1]:.3e}, Gauss-Newton {eg[0]:.3e} {eg[1]:.3e}')
        if kind == 'noise':
            assert eg[0] < eh[0] and eg[1] < eh[1]
        else:
            assert eh[0] < 1e-5 and eh[1] < 1e-5              # the closed form in the test is a sound yardstick


@pytest.mark.parametrize('case', PI.CASES, ids=PI.case_id)
def test_conditions_the_gpu_test_rests_on(case):
    """the GPU test compares counts and status exactly with the float32 restatement and floats with the float64 one inside
    pose_ref.tolerance: that only means something while the two restatements agree on the counts and the tolerance stays small"""
    shape, kind = case
    for pi in range(len(PI.PARAMS)):
        r32, r64 = PI.refs(shape, kind, pi)
        assert np.array_equal(r32['n_used'], r64['n_used'])
        assert np.array_equal(r32['stats'][..., 0], r64['stats'][..., 0]) and np.array_equal(r32['stats'][..., 3], r64['stats'][..., 3])
        for k in ('R_pair', 't_pair'):
            allowed = pose_ref.tolerance(r32[k], r64[k])
            print(f'params {pi} {k}: tolerance {allowed:.3e}, max |ref32 - ref64| {float(np.abs(r32[k] - r64[k]).max()):.3e}')
            assert allowed <= 1e-4
        assert np.all(np.isfinite(r64['R_pair'])) and np.all(np.isfinite(r64['t_pair'])) and np.all(np.isfinite(r64['stats']))


@pytest.mark.parametrize('case', [(SMALLEST, 'plane'), (SMALLEST, 'noise'), (PI.SHAPES[1], 'no_overlap'), (PI.SHAPES[3], 'no_overlap')],
                         ids=PI.case_id)
def test_a_pair_without_enough_pixels_fails_and_stays_at_the_identity(case):
    shape, kind = case
    n, tl, H, W = shape
    for dt in range(2):
        r = PI.refs(shape, kind, 0)[dt]
        off = _offdiag(tl)
        assert np.all(r['stats'][:, off, 3] == 0) and np.all(r['stats'][:, ~off] == np.array([0, 0, 0, 1]))
        assert np.all(r['R_pair'] == np.eye(3)) and np.all(r['t_pair'] == 0) and np.all(r['steps'] == 0)
        if kind == 'no_overlap':
            assert np.all(r['stats'][..., :3] == 0)
        else:
            assert np.all(r['stats'][:, off, 0] <= H * W)


def test_holes_and_bad_flows_only_remove_pixels():
    shape = PI.SHAPES[3]
    full = PI.refs(shape, 'plane', 0)[1]['stats'][..., 0]
    for kind in ('holes', 'nan_flow'):
        a, r = PI.make_input(shape, kind), PI.refs(shape, kind, 0)[1]
        off = _offdiag(shape[1])
        assert np.all(r['stats'][:, off, 0] < full[:, off]) and np.all(r['stats'][:, off, 0] >= PI.MIN_CORR)
        assert PI.pose_error(r, a)[0] <= pose_ref.tolerance(PI.refs(shape, kind, 0)[0]['R_pair'], r['R_pair'])


# ------------------------------------------------------------------------------------------------ data/presave_pose.py, data/convert.py
def _rot(w):
    from depthinspace_amd import synth
    return synth._rodrigues(np.asarray(w, dtype=np.float64))


def _hand_made_track(tl=4, seed=3):
    from depthinspace_amd.data import presave_pose as PP
    rng = np.random.RandomState(seed)
    R = np.stack([np.eye(3)] + [_rot(rng.uniform(-0.1, 0.1, 3)) for _ in range(tl - 1)])
    t = np.concatenate([np.zeros((1, 3)), rng.uniform(-0.2, 0.2, (tl - 1, 3))])
    Rp, tp = PP.relative_poses(R, t)
    return R, t, Rp, tp


def test_relative_poses_and_their_composition():
    from depthinspace_amd.data import presave_pose as PP
    R, t, Rp, tp = _hand_made_track()
    tl = len(R)
    X = np.random.RandomState(1).normal(size=(5, 3))
    for i in range(tl):
        for j in range(tl):
            Xi, Xj = X @ R[i].T + t[i], X @ R[j].T + t[j]
            assert np.allclose(Xi @ Rp[i, j].T + tp[i, j], Xj, atol=1e-14)
    assert np.allclose(Rp[0, 2], PI.pair_truth(R[None], t[None])[0][0, 0, 2], atol=1e-15)
    ok = np.ones((tl, tl), bool)
    got = PP.compose_track(Rp, tp, ok)
    assert got[0].dtype == np.float32 and got[0].shape == (tl, 3, 3) and got[1].shape == (tl, 3)
    assert np.array_equal(got[0][0], np.eye(3)) and np.array_equal(got[1][0], np.zeros(3))
    assert np.array_equal(got[0], R.astype(np.float32)) and np.array_equal(got[1], t.astype(np.float32))
    # pair (0, 2) failed: frame 2 comes from the inverse of pair (2, 0), and the forward pair is not read
    ok[0, 2] = False
    broken_R, broken_t = Rp.copy(), tp.copy()
    broken_R[0, 2], broken_t[0, 2] = np.nan, np.nan
    got = PP.compose_track(broken_R, broken_t, ok)
    assert np.allclose(got[0], R, atol=1e-7) and np.allclose(got[1], t, atol=1e-7)
    ok[2, 0] = False
    assert PP.compose_track(broken_R, broken_t, ok) is None
    ok[:] = True
    ok[1:, :] = False                                          # only the pairs from frame 0 are needed
    assert PP.compose_track(Rp, tp, ok) is not None


def test_report_arithmetic():
    from depthinspace_amd.data import presave_pose as PP
    assert abs(float(PP.rotation_angle(_rot([0, 0, 1e-9]))) - 1e-9) < 1e-15 and abs(float(PP.rotation_angle(_rot([0.3, -0.4, 1.2]))) - 1.3) < 1e-12
    assert PP.median_depth(np.array([[2.0, 0.0, np.nan, 4.0, -1.0, np.inf, 8.0]]), 8.0) == 2.0
    assert np.isnan(PP.median_depth(np.zeros((2, 2)), 8.0))
    R, t, Rp, tp = _hand_made_track(tl=3)
    stats = np.zeros((3, 3, 4))
    stats[..., 0], stats[..., 1], stats[..., 2], stats[..., 3] = 50, 0.5, 0.25, 1
    stats[np.eye(3, dtype=bool)] = [0, 0, 0, 1]
    exact = PP.report_terms(Rp, tp, stats, pixels=100, depth=3.0, stored=(R, t))
    assert exact['ok'] == 6 and exact['failed'] == 0 and exact['cycles'] == 3 and exact['gt_pairs'] == 6
    assert abs(exact['share'] - 3.0) < 1e-12 and abs(exact['weight'] - 3.0) < 1e-12 and abs(exact['resid'] - 1.5) < 1e-12
    assert max(exact['cycle_rot'], exact['cycle_trans'], exact['gt_rot'], exact['gt_trans']) < 1e-12
    # one pair turned by 0.01 rad, another one shifted by 0.3 at depth 3: each shows in the cycle of its pair and against the stored poses
    Rq, tq = Rp.copy(), tp.copy()
    Rq[0, 1] = _rot([0, 0, 0.01]) @ Rp[0, 1]
    tq[2, 1] = tp[2, 1] + np.array([0.3, 0, 0])
    r = PP.report_terms(Rq, tq, stats, pixels=100, depth=3.0, stored=(R, t))
    assert abs(r['cycle_rot'] - 0.01) < 1e-12 and abs(r['gt_rot'] - 0.01) < 1e-12
    turn = np.linalg.norm(tp[1, 0] + Rp[1, 0] @ tq[0, 1]) / 3.0     # (turning R_01 leaves t_10 + R_10 t_01 as it was: zero)
    assert turn < 1e-12 and abs(r['cycle_trans'] - 0.1) < 1e-12 and abs(r['gt_trans'] - 0.1) < 1e-12
    # a failed direction leaves the ordered-pair sums and takes its unordered pair out of the cycles
    stats[0, 2, 3] = 0
    f = PP.report_terms(Rq, tq, stats, pixels=100, depth=3.0)
    assert f['ok'] == 5 and f['failed'] == 1 and f['cycles'] == 2 and 'gt_pairs' not in f and abs(f['share'] - 2.5) < 1e-12
    line = PP.report_line({k: 2 * v for k, v in r.items()})         # two such tracks
    assert line['ok'] == 12 and abs(line['share'] - 0.5) < 1e-12 and abs(line['cycle_rot'] - 0.01 / 3) < 1e-12
    assert abs(line['gt_trans'] - 0.1 / 6) < 1e-12 and abs(line['resid'] - 0.25) < 1e-12
    assert np.isnan(PP.report_line({'ok': 0, 'failed': 2, 'share': 0.0, 'weight': 0.0, 'resid': 0.0, 'cycles': 0, 'cycle_rot': 0.0,
                                    'cycle_trans': 0.0})['share'])


def test_loaders_follow_the_rules_of_the_fusion_stage(tmp_path):
    from depthinspace_amd.data import presave_pose as PP
    d = str(tmp_path)
    disp = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 1, 3, 4)
    np.savez(os.path.join(d, 'frames.npz'), im=disp, disp=disp, sgm_disp=disp + 1)
    np.savez(os.path.join(d, 'multi_frame_disp.npz'), disp=disp + 2)
    assert np.array_equal(PP.load_disp(d, 'gt'), disp[:, 0]) and np.array_equal(PP.load_disp(d, 'sgm'), disp[:, 0] + 1)
    assert np.array_equal(PP.load_disp(d, 'multi_frame'), disp[:, 0] + 2) and PP.stored_poses(d) is None
    with pytest.raises(ValueError):
        PP.load_disp(d, 'single_frame')
    with pytest.raises(ValueError):
        PP.load_disp(d, 'other')
    with pytest.raises(ValueError):
        PP.load_flow(d, 2)
    f01, f10 = np.full((1, 2, 3, 4), 1.5, np.float32), np.full((1, 2, 3, 4), -2.5, np.float32)
    np.savez(os.path.join(d, 'flow.npz'), flow_01=f01, flow_10=f10)
    flow = PP.load_flow(d, 2)
    assert flow.shape == (4, 2, 3, 4) and np.all(flow[0] == 0) and np.all(flow[3] == 0) and np.all(flow[1] == 1.5) and np.all(flow[2] == -2.5)


def test_a_track_without_poses_converts_when_asked_to(tmp_path):
    from depthinspace_amd import synth
    from depthinspace_amd.data import convert
    from tests.test_dataset_cpu import _FakeH5
    st = synth.make_settings(32, 24)
    b = synth.make_batch(st, 1, 4, seed=40, with_primary=False, with_flow=False)
    im = b['im0'][0]
    src = tmp_path / 'ref' / '00000000'
    src.mkdir(parents=True)
    store = {str(src / 'frames.hdf5'): _FakeH5(im=im, ambient=b['ambient0'][0], grad=np.zeros_like(im), disp=b['disp0'][0])}
    open(str(src / 'frames.hdf5'), 'wb').close()
    with pytest.raises(KeyError):                                  # the default is what it was
        convert.convert_track(str(src), str(tmp_path / 'a'), open_h5=lambda p: store[p])
    assert convert.convert_track(str(src), str(tmp_path / 'b'), open_h5=lambda p: store[p], require_poses=False) == ['frames.npz']
    with np.load(str(tmp_path / 'b' / 'frames.npz')) as f:
        assert sorted(f.files) == ['ambient', 'disp', 'grad', 'im'] and np.array_equal(f['im'], im)
    store[str(src / 'frames.hdf5')].pop('disp')                    # the other arrays stay mandatory
    with pytest.raises(KeyError):
        convert.convert_track(str(src), str(tmp_path / 'c'), open_h5=lambda p: store[p], require_poses=False)
