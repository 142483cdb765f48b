"""GPU, end to end: the model stage of data/presave_pose.py (frame-to-model refinement, ops.tsdf_align_poses) on a small rendered
root - model_refine_track from perturbed true poses, and presave_pose --joint --model --report against the same command without
--model."""
import os
import re

import numpy as np
import pytest

from tests import pose_inputs as PI
from tests import tsdf_align_inputs as AI
from tests import tsdf_align_ref as AR

pytestmark = pytest.mark.gpu

H, W = 64, 96
RES = 64
MODEL_KEYS = ('model_resid_before', 'model_resid_after', 'model_used', 'model_failed', 'model_gt_rot', 'model_gt_trans')


def _arrays(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _bytes(path):
    with open(path, 'rb') as fp:
        return fp.read()


def _root(tmp_path, poses):
    """two rendered tracks of four frames on disk, with their flows; poses: whether frames.npz stores R and t"""
    from depthinspace_amd.data import dataset as D
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    shape = (2, 4, H, W)
    a = PI.make_input(shape, 'render')                              # render_scenes.small_scene(11), (12) through tests/render_ref.py
    tl = shape[1]
    root = str(tmp_path / 'data')
    D.save_settings(root, st)
    paths = []
    for b in range(shape[0]):
        d = os.path.join(root, f'{b:08d}')
        os.makedirs(d)
        disp = a['disp'][b][:, None]
        extra = {'R': a['R'][b], 't': a['t'][b]} if poses else {}
        np.savez(os.path.join(d, 'frames.npz'), im=disp, ambient=disp, grad=np.zeros_like(disp), disp=disp, **extra)
        np.savez(os.path.join(d, 'flow.npz'), **{f'flow_{i}{j}': a['flow'][b, i * tl + j][None] for i in range(tl) for j in range(tl) if i != j})
        paths.append(d)
    return root, paths, a, st


def test_model_refine_track_from_perturbed_true_poses():
    from depthinspace_amd.data import mesh, presave_pose as PP
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    a = PI.make_input((2, 4, H, W), 'render')
    disp, Rt, tt = a['disp'][0], a['R'][0], a['t'][0]
    tl = len(Rt)
    origin, voxel, trunc, grid = mesh.place_track(disp, Rt, tt, None, st, res=RES)
    centre = AI.centre_of(origin, voxel, grid)
    R0, t0 = Rt.copy(), tt.copy()
    for f in range(1, tl):                                          # frame 0 stays the world
        R0[f], t0[f] = AI.perturb(Rt[f], tt[f], centre, voxel, f, mag=0.7)
    r = PP.model_refine_track(disp, R0, t0, None, st, rounds=2, iters=6, res=RES)
    assert r is not None and np.array_equal(r['R'][0], R0[0]) and np.array_equal(r['t'][0], t0[0])
    assert r['R'].dtype == np.float32 and r['R'].shape == (tl, 3, 3) and r['t'].shape == (tl, 3) and not r['first'][0].any()
    for f in range(1, tl):
        e0, e1 = AR.pose_error(R0[f], t0[f], Rt[f], tt[f]), AR.pose_error(r['R'][f], r['t'][f], Rt[f], tt[f])
        before, after = r['first'][f, 6] / r['voxel'], r['last'][f, 2] / r['voxel']
        print(f'frame {f}: rms distance to the model {before:.3f} -> {after:.3f} voxels, rotation {np.rad2deg(e0[0]):.3f} -> {np.rad2deg(e1[0]):.3f} deg, '
              f'translation {e0[1] / r["voxel"]:.3f} -> {e1[1] / r["voxel"]:.3f} voxels, used {int(r["last"][f, 0])} of {int(r["last"][f, 7])}')
        assert r['first'][f, 3] == 1 and r['last'][f, 3] == 1
        assert after < before and e1[0] < e0[0] and e1[1] < e0[1]


def test_presave_pose_joint_model_report(tmp_path, capsys):
    from depthinspace_amd.data import presave_pose as PP
    root, paths, a, st = _root(tmp_path, poses=True)
    before = {p: _arrays(os.path.join(p, 'frames.npz')) for p in paths}
    flows = {p: _bytes(os.path.join(p, 'flow.npz')) for p in paths}
    capsys.readouterr()
    PP.main([root, '--disp', 'gt', '--joint', '--model', '--report', '--force', '--res', str(RES)])
    out = capsys.readouterr().out
    print(out)
    rep = {k: float(v) for k, v in re.findall(r'(\w+) (-?[0-9.]+(?:e[-+]?[0-9]+)?|nan)(?:  |\n|$)', out)}
    assert all(k in rep and np.isfinite(rep[k]) for k in MODEL_KEYS + ('joint_gt_rot', 'gt_rot')), rep
    assert rep['model_failed'] == 0 and 0 < rep['model_used'] <= 1 and 0 < rep['model_resid_after'] <= rep['model_resid_before']
    assert 'model rounds 2 iters 6' in out and '2 tracks written' in out
    for p in paths:
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz'] and _bytes(os.path.join(p, 'flow.npz')) == flows[p]
        after = _arrays(os.path.join(p, 'frames.npz'))
        assert sorted(after) == sorted(before[p])
        for k, v in before[p].items():
            if k not in ('R', 't'):
                assert after[k].dtype == v.dtype and after[k].shape == v.shape and after[k].tobytes() == v.tobytes(), k
        R, t = after['R'], after['t']
        assert R.dtype == np.float32 and R.shape == (4, 3, 3) and t.dtype == np.float32 and t.shape == (4, 3)
        assert np.array_equal(R[0], np.eye(3)) and np.array_equal(t[0], np.zeros(3)) and np.isfinite(R).all() and np.isfinite(t).all()
    with_model = {p: _arrays(os.path.join(p, 'frames.npz')) for p in paths}
    # the same command without --model: the joint poses, as ops.refine_track_poses gives them from the chained pairwise result
    capsys.readouterr()
    PP.main([root, '--disp', 'gt', '--joint', '--report', '--force'])
    out = capsys.readouterr().out
    assert 'model rounds' not in out and not any(k in out for k in MODEL_KEYS)
    disps = [PP.load_disp(p, 'gt') for p in paths]
    fl = [PP.load_flow(p, 4) for p in paths]
    Rp, tp, stats = PP.estimate_pairs(disps, fl, st)
    ok = stats[..., 3] != 0
    starts = [PP.chain_track(Rp[b], tp[b], ok[b]) for b in range(2)]
    Rj, tj, _, jst = PP.refine_tracks(disps, fl, st, np.stack([s[0] for s in starts]), np.stack([s[1] for s in starts]), ok)
    assert np.all(jst[:, 3] == 1)
    for b, p in enumerate(paths):
        after = _arrays(os.path.join(p, 'frames.npz'))
        assert after['R'].tobytes() == Rj[b].tobytes() and after['t'].tobytes() == tj[b].tobytes()
        assert after['R'].tobytes() != with_model[p]['R'].tobytes()          # the model stage had moved them
        for k, v in before[p].items():
            if k not in ('R', 't'):
                assert after[k].tobytes() == v.tobytes(), k
