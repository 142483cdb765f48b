"""GPU, end to end: rendered tracks on disk, their poses removed -> python -m depthinspace_amd.data.presave_pose (ops.track_poses on the
stored disparities and flows) -> R and t back in frames.npz, good enough for the readers and for the fusion stage."""
import os
import shutil

import numpy as np
import pytest

from tests import pose_ref

pytestmark = pytest.mark.gpu

H, W = 64, 48


def _bytes(path):
    with open(path, 'rb') as fp:
        return fp.read()


def _arrays(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _strip_poses(d):
    """frames.npz without R and t -> the poses it held"""
    a = _arrays(os.path.join(d, 'frames.npz'))
    R, t = a.pop('R'), a.pop('t')
    np.savez(os.path.join(d, 'frames.npz'), **a)
    return R, t


def _report_numbers(line):
    tok = line.split(': ', 1)[1].split()
    return {tok[k]: float(tok[k + 1]) for k in range(0, len(tok) - 1, 2)}


def test_presave_pose_command_on_rendered_tracks(tmp_path, capsys):
    from depthinspace_amd.data import dataset as D, fuse as F, presave_pose as PP, render
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    root, root_true = str(tmp_path / 'data'), str(tmp_path / 'true')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    shutil.copytree(root, root_true)
    truth = [_strip_poses(p) for p in paths]
    before = {p: _arrays(os.path.join(p, 'frames.npz')) for p in paths}
    flows = {p: _bytes(os.path.join(p, 'flow.npz')) for p in paths}
    settings_before = _bytes(os.path.join(root, 'settings.npz'))
    with pytest.raises(KeyError):
        F.fuse_dataset(root, 'gt')                                  # where the chain stopped for a track without poses
    capsys.readouterr()
    PP.main([root, '--disp', 'gt', '--report'])
    out = capsys.readouterr().out
    print(out)
    assert '2 tracks written' in out and 'failed and were left' not in out
    rep = _report_numbers([l for l in out.split('\n') if l.startswith('poses from the gt')][0])
    tl = len(truth[0][0])
    assert rep['tracks'] == 2 and rep['written'] == 2 and rep['failed_tracks'] == 0 and rep['ok'] == 2 * tl * (tl - 1) and rep['failed'] == 0
    assert 0 < rep['share'] <= 1 and 0 < rep['weight'] <= 1 and rep['resid'] >= 0 and 'gt_rot' not in rep     # no poses were stored
    assert _bytes(os.path.join(root, 'settings.npz')) == settings_before
    for p, (Rt, tt) in zip(paths, truth):
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz']                        # no temporary file is left
        assert _bytes(os.path.join(p, 'flow.npz')) == flows[p]
        after = _arrays(os.path.join(p, 'frames.npz'))
        assert sorted(after) == sorted(list(before[p]) + ['R', 't'])
        for k, v in before[p].items():
            assert after[k].dtype == v.dtype and after[k].shape == v.shape and after[k].tobytes() == v.tobytes(), k
        R, t = after['R'], after['t']
        assert R.dtype == np.float32 and R.shape == (tl, 3, 3) and t.dtype == np.float32 and t.shape == (tl, 3)
        assert np.array_equal(R[0], np.eye(3)) and np.array_equal(t[0], np.zeros(3))        # frame 0 is the world
        # the pairs (0, j) against the rendered truth: no further off than the float64 restatement on the same arrays, plus what the
        # device may deviate from it
        disp, flow = PP.load_disp(p, 'gt'), PP.load_flow(p, tl)
        r32, r64 = (pose_ref.track_poses(disp[None], flow[None], st.K, st.baseline, dtype=dt) for dt in (np.float32, np.float64))
        assert np.all(r64['stats'][..., 3] == 1)
        Rp, tp = PP.relative_poses(Rt, tt)
        for name, got, ref32, ref64, true in (('R', R, r32['R_pair'][0, 0], r64['R_pair'][0, 0], Rp[0]),
                                              ('t', t, r32['t_pair'][0, 0], r64['t_pair'][0, 0], tp[0])):
            own = float(np.abs(ref64 - true).max())
            err = float(np.abs(got.astype(np.float64) - true).max())
            allowed = own + pose_ref.tolerance(ref32, ref64)
            print(f'{p} {name}: max |stored - truth| {err:.3e}, the float64 restatement {own:.3e}, allowed {allowed:.3e}')
            assert err <= allowed
    # a second run writes nothing; --force rewrites the same bytes
    files = {p: _bytes(os.path.join(p, 'frames.npz')) for p in paths}
    stamp = {p: os.stat(os.path.join(p, 'frames.npz')).st_mtime_ns for p in paths}
    assert PP.presave_pose(root, 'gt') == 0
    assert all(os.stat(os.path.join(p, 'frames.npz')).st_mtime_ns == stamp[p] for p in paths)
    capsys.readouterr()
    PP.main([root, '--disp', 'gt', '--force', '--report'])
    out = capsys.readouterr().out
    print(out)
    assert '2 tracks written' in out
    again = _report_numbers([l for l in out.split('\n') if l.startswith('poses from the gt')][0])
    assert 'gt_rot' in again and 'gt_trans' in again                        # this time poses were stored: those of the first run
    assert all(_bytes(os.path.join(p, 'frames.npz')) == files[p] for p in paths)
    with pytest.raises(ValueError):
        PP.presave_pose(root, 'sgm', force=True)                      # no sgm_disp stored
    # the readers take the result
    ds = D.TrackNpzDataset(root, paths, tl, train=False, load_flow_data=True)
    s = ds[1]
    assert np.array_equal(s['R'].numpy(), _arrays(os.path.join(paths[1], 'frames.npz'))['R']) and tuple(s['t'].shape) == (tl, 3)
    # and the fusion stage finds the surfaces of the frames on each other, as with the true poses
    est = F.fuse_dataset(root, 'gt', report=True)
    true = F.fuse_dataset(root_true, 'gt', report=True)
    print(capsys.readouterr().out, f'consistent: estimated poses {est["consistent"]:.6f}, true poses {true["consistent"]:.6f}')
    assert est['consistent'] > 0.5 and est['tracks'] == 2
    # the report on the rendered tracks themselves: nothing is written, the estimate is measured against the stored poses
    stored = {p: _bytes(os.path.join(p, 'frames.npz')) for p in (os.path.join(root_true, os.path.basename(q)) for q in paths)}
    rep = PP.presave_pose(root_true, 'gt', report=True)
    print(capsys.readouterr().out)
    assert rep['written'] == 0 and rep['tracks'] == 2 and np.isfinite(rep['gt_rot']) and np.isfinite(rep['gt_trans'])
    assert np.isfinite(rep['cycle_rot']) and np.isfinite(rep['cycle_trans'])
    assert all(_bytes(p) == b for p, b in ((os.path.join(p, 'frames.npz'), b) for p, b in stored.items()))


def test_a_track_whose_flows_leave_the_image_is_reported_and_left_untouched(tmp_path, capsys):
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, presave_pose as PP
    from tests import pose_inputs as PI
    shape = PI.SHAPES[2]
    n, tl, h, w = shape
    root = str(tmp_path / 'data')
    D.save_settings(root, synth.make_settings(h, w))
    files = {}
    for b, kind in enumerate(('no_overlap', 'bumps')):
        a = PI.make_input(shape, kind)
        d = os.path.join(root, f'{b:08d}')
        os.makedirs(d)
        disp = a['disp'][b][:, None]
        np.savez(os.path.join(d, 'frames.npz'), im=disp, ambient=disp, grad=np.zeros_like(disp), disp=disp)
        np.savez(os.path.join(d, 'flow.npz'), **{f'flow_{i}{j}': a['flow'][b, i * tl + j][None] for i in range(tl) for j in range(tl) if i != j})
        files[d] = _bytes(os.path.join(d, 'frames.npz'))
    rep = PP.presave_pose(root, 'gt', report=True)
    out = capsys.readouterr().out
    print(out)
    bad, good = sorted(files)
    assert rep['tracks'] == 2 and rep['written'] == 1 and rep['failed_tracks'] == 1 and rep['ok'] == tl * (tl - 1) == rep['failed']
    assert '1 tracks failed' in out and os.path.basename(bad) in out.split('left as they are: ')[1].split('\n')[0]
    assert _bytes(os.path.join(bad, 'frames.npz')) == files[bad] and sorted(os.listdir(bad)) == ['flow.npz', 'frames.npz']
    R = _arrays(os.path.join(good, 'frames.npz'))['R']
    r32, r64 = PI.refs(shape, 'bumps', 0)
    true = PI.make_input(shape, 'bumps')['R_pair'][1, 0, 1:]
    allowed = float(np.abs(r64['R_pair'][1, 0, 1:] - true).max()) + pose_ref.tolerance(r32['R_pair'][1, 0, 1:], r64['R_pair'][1, 0, 1:])
    assert np.array_equal(R[0], np.eye(3)) and float(np.abs(R.astype(np.float64)[1:] - true).max()) <= allowed
