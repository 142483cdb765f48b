"""GPU, end to end: rendered tracks on disk without poses, the flows of two pairs of one track broken -> presave_pose as it was
(the composed pairwise poses) -> presave_pose --joint (ops.refine_track_poses on top): the broken pair no longer sets the stored pose."""
import os

import numpy as np
import pytest

from tests import pose_inputs as PI
from tests import pose_joint_inputs as JI
from tests import pose_joint_ref as JR
from tests import pose_ref
from tests.test_pose_pipeline_gpu import _arrays, _bytes

pytestmark = pytest.mark.gpu

H, W = 64, 96
JOINT_KEYS = ('joint_resid', 'joint_share', 'joint_failed', 'joint_gt_rot', 'joint_gt_trans')


def _pair_error(R, t, Rt, tt):
    """max |R_pair - truth|, max |t_pair - truth| over all pairs of the poses R, t against the poses Rt, tt"""
    a = {k: v for k, v in zip(('R_pair', 't_pair'), PI.pair_truth(Rt[None], tt[None]))}
    return JI.pose_error(R[None], t[None], a)


def _device_pairs(PP, p, tl, st):
    import torch
    from depthinspace_amd import ops
    disp, flow = PP.load_disp(p, 'gt'), PP.load_flow(p, tl)
    r = ops.track_poses(torch.from_numpy(disp[None]).cuda(), torch.from_numpy(flow[None]).cuda(), st.K, st.baseline)
    return tuple(r[k][0].cpu().numpy() for k in ('R_pair', 't_pair', 'stats'))


def test_presave_pose_joint_on_rendered_tracks(tmp_path, capsys):
    from depthinspace_amd.data import dataset as D, presave_pose as PP
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    shape = (2, 4, H, W)
    n, tl = shape[:2]
    a = PI.make_input(shape, 'render')                              # render_scenes.small_scene(11), (12) through tests/render_ref.py
    flow = a['flow'].copy()
    flow[1:] = JI.break_flows(flow[1:], tl)                         # track 1: the pairs (0, 2) and (2, 0) broken
    root = str(tmp_path / 'data')
    D.save_settings(root, st)
    paths, truth = [], []
    for b in range(n):
        d = os.path.join(root, f'{b:08d}')
        os.makedirs(d)
        disp = a['disp'][b][:, None]
        np.savez(os.path.join(d, 'frames.npz'), im=disp, ambient=disp, grad=np.zeros_like(disp), disp=disp)   # no R, no t
        np.savez(os.path.join(d, 'flow.npz'), **{f'flow_{i}{j}': flow[b, i * tl + j][None] for i in range(tl) for j in range(tl) if i != j})
        paths.append(d)
        truth.append((a['R'][b], a['t'][b]))
    before = {p: _arrays(os.path.join(p, 'frames.npz')) for p in paths}
    flows = {p: _bytes(os.path.join(p, 'flow.npz')) for p in paths}
    # 1. without joint: what it writes today, the composed pairs of ops.track_poses
    assert PP.presave_pose(root, source='gt') == 2
    pairwise = []
    for p in paths:
        Rp, tp, stats = _device_pairs(PP, p, tl, st)
        assert np.all(stats[..., 3] == 1)                          # the broken pairs still report ok
        want = PP.compose_track(Rp, tp, stats[..., 3] != 0)
        after = _arrays(os.path.join(p, 'frames.npz'))
        assert after['R'].tobytes() == want[0].tobytes() and after['t'].tobytes() == want[1].tobytes()
        pairwise.append((after['R'], after['t']))
    # 2. with joint
    capsys.readouterr()
    rep = PP.presave_pose(root, source='gt', joint=True, force=True, report=True)
    out = capsys.readouterr().out
    print(out)
    assert rep['tracks'] == 2 and rep['written'] == 2 and rep['failed_tracks'] == 0 and rep['joint_failed'] == 0
    assert all(k in rep and np.isfinite(rep[k]) for k in JOINT_KEYS) and 'gt_rot' in rep and 'joint iters 6' in out
    assert 0 < rep['joint_share'] <= 1 and rep['joint_resid'] > 0
    for b, (p, (Rt, tt)) in enumerate(zip(paths, truth)):
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz'] and _bytes(os.path.join(p, 'flow.npz')) == flows[p]
        after = _arrays(os.path.join(p, 'frames.npz'))
        assert sorted(after) == sorted(list(before[p]) + ['R', 't'])
        for k, v in before[p].items():
            assert after[k].dtype == v.dtype and after[k].shape == v.shape and after[k].tobytes() == v.tobytes(), k
        R, t = after['R'], after['t']
        assert R.dtype == np.float32 and R.shape == (tl, 3, 3) and t.dtype == np.float32 and t.shape == (tl, 3)
        assert np.array_equal(R[0], np.eye(3)) and np.array_equal(t[0], np.zeros(3))
        pw, jt = _pair_error(*pairwise[b], Rt, tt), _pair_error(R, t, Rt, tt)
        print(f'{p}: pairwise R {pw[0]:.3e} t {pw[1]:.3e}, joint R {jt[0]:.3e} t {jt[1]:.3e}')
        if b == 1:                                                  # the condition of tests/test_pose_joint_ref_cpu.py
            assert jt[0] <= 0.5 * pw[0] and jt[1] <= 0.5 * pw[1]
        else:
            disp, flow = PP.load_disp(p, 'gt'), PP.load_flow(p, tl)
            r32, r64 = (pose_ref.track_poses(disp[None], flow[None], st.K, st.baseline, dtype=dt) for dt in (np.float32, np.float64))
            assert jt[0] <= pw[0] + pose_ref.tolerance(r32['R_pair'], r64['R_pair'])
            assert jt[1] <= pw[1] + pose_ref.tolerance(r32['t_pair'], r64['t_pair'])
    # the pairwise figures of the report are those of a run without joint
    plain = PP.presave_pose(root, source='gt', report=True)
    assert all(k not in plain for k in JOINT_KEYS)
    for k in ('ok', 'failed', 'share', 'weight', 'resid', 'cycle_rot', 'cycle_trans'):
        assert plain[k] == rep[k], k


def test_a_frame_without_a_pair_with_frame_0_is_reached_through_the_others(tmp_path, capsys):
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, presave_pose as PP
    shape = PI.SHAPES[3]
    n, tl, h, w = shape
    a = PI.make_input(shape, 'bumps')
    flow = a['flow'].copy()
    for (i, j) in JI.BROKEN_PAIRS:
        flow[:, i * tl + j] += np.float32(2 * w)                    # these two pairs fail: no pixel has a target
    root = str(tmp_path / 'data')
    D.save_settings(root, synth.make_settings(h, w))
    d = os.path.join(root, '00000000')
    os.makedirs(d)
    disp = a['disp'][0][:, None]
    np.savez(os.path.join(d, 'frames.npz'), im=disp, ambient=disp, grad=np.zeros_like(disp), disp=disp)
    np.savez(os.path.join(d, 'flow.npz'), **{f'flow_{i}{j}': flow[0, i * tl + j][None] for i in range(tl) for j in range(tl) if i != j})
    kept = _bytes(os.path.join(d, 'frames.npz'))
    rep = PP.presave_pose(root, 'gt', report=True)
    assert rep['written'] == 0 and rep['failed_tracks'] == 1 and rep['failed'] == 2 and _bytes(os.path.join(d, 'frames.npz')) == kept
    rep = PP.presave_pose(root, 'gt', report=True, joint=True)
    print(capsys.readouterr().out)
    assert rep['written'] == 1 and rep['failed_tracks'] == 0 and rep['joint_failed'] == 0 and rep['failed'] == 2
    assert abs(rep['joint_share'] - 10 / 12) < 1e-6
    got = _arrays(os.path.join(d, 'frames.npz'))
    # the same stage in numpy: the float64 pairwise restatement, chained, refined on the ok pairs
    pw = pose_ref.track_poses(a['disp'], flow, a['K'], a['baseline'], *PI.PARAMS[0], PI.MIN_CORR, dtype=np.float64)
    ok = pw['stats'][0, ..., 3] != 0
    assert not ok[0, 2] and not ok[2, 0] and ok.sum() == tl + 10
    R0, t0 = PP.chain_track(pw['R_pair'][0], pw['t_pair'][0], ok)
    r32, r64 = (JR.refine_track_poses(a['disp'], flow, a['K'], a['baseline'], R0[None], t0[None], ok[None], *PI.PARAMS[0], PI.MIN_CORR, dtype=dt)
                for dt in (np.float32, np.float64))
    for k in ('R', 't'):
        err, allowed = float(np.abs(got[k].astype(np.float64) - r64[k][0]).max()), pose_ref.tolerance(r32[k], r64[k])
        print(f'{k}: max |stored - ref64| {err:.3e}, allowed {allowed:.3e}')
        assert err <= allowed
    e = JI.pose_error(got['R'][None], got['t'][None], a)
    own = JI.pose_error(r64['state_R'], r64['state_t'], a)
    assert e[0] <= own[0] + pose_ref.tolerance(r32['R'], r64['R']) and e[1] <= own[1] + pose_ref.tolerance(r32['t'], r64['t'])
