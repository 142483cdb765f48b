"""GPU, end to end: rendered tracks on disk -> python -m depthinspace_amd.data.raycast (the placement and integration of data/mesh.py,
then ops.tsdf_raycast into the track's own frames) -> raycast_<disp>.npz per track, and the report."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, RES = 64, 48, 48


def _bytes(path):
    with open(path, 'rb') as fp:
        return fp.read()


def _report_numbers(line):
    tok = line.split(': ', 1)[1].split()
    return {tok[k]: float(tok[k + 1]) for k in range(0, len(tok) - 1, 2)}


def test_raycast_command_on_rendered_tracks(tmp_path, capsys):
    from depthinspace_amd import ops
    from depthinspace_amd.data import mesh as M, raycast as RC, render
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    before = {p: {f: _bytes(os.path.join(p, f)) for f in os.listdir(p)} for p in paths}
    settings_before = _bytes(os.path.join(root, 'settings.npz'))
    capsys.readouterr()
    RC.main([root, '--disp', 'gt', '--res', str(RES), '--report'])
    out = capsys.readouterr().out
    print(out)
    assert '2 raycast files written' in out
    rep = _report_numbers([l for l in out.split('\n') if l.startswith('raycast of the gt')][0])
    assert set(rep) == {'tracks', 'written', 'hit', 'kept', 'moved'}                      # gt against itself: no gt terms
    assert rep['tracks'] == 2 and rep['written'] == 2 and 0 < rep['hit'] <= 1 and 0 < rep['kept'] <= 1 and 0 <= rep['moved'] < 1
    hit = pixels = 0
    fb = float(st.K[0][0]) * float(st.baseline)
    for p in paths:
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz', 'raycast_gt.npz']       # no temporary file is left
        for f, b in before[p].items():
            assert _bytes(os.path.join(p, f)) == b, f
        with np.load(os.path.join(p, 'raycast_gt.npz')) as f:
            assert sorted(f.files) == ['disp', 'normal', 'value']
            got = {k: f[k] for k in f.files}
        with np.load(os.path.join(p, 'frames.npz')) as f:
            disp, R, t, amb = f['disp'][:, 0], f['R'], f['t'], f['ambient'][:, 0]
        tl = disp.shape[0]
        assert got['disp'].shape == (tl, 1, H, W) and got['normal'].shape == (tl, 3, H, W) and got['value'].shape == (tl, 1, H, W)
        assert all(v.dtype == np.float32 for v in got.values())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        # a direct call with the same placement
        r = ops.fuse_track(up(disp)[None], up(R)[None], up(t)[None], st.K, st.baseline, up(amb)[None], tol=0.01, min_views=2)
        m = int(r['count'].sum().item())
        assert m > 0
        origin, voxel, trunc, grid = M.place_volume(r['xyz'][:m], RES, None, 3.0)
        vol = ops.tsdf_integrate(up(disp), up(R), up(t), st.K, st.baseline, up(amb), origin=origin, voxel=voxel, trunc=trunc, grid=grid)
        g = ops.tsdf_raycast(vol[0], vol[1], vol[2], origin, voxel, up(R), up(t), st.K, st.baseline, size=(H, W))
        assert np.array_equal(got['disp'][:, 0], g['disp'].cpu().numpy()) and np.array_equal(got['normal'], g['normal'].cpu().numpy())
        assert np.array_equal(got['value'][:, 0], g['value'].cpu().numpy())
        # the surface lies within a voxel of the disparities it was made from: the median relative error is within a voxel of depth
        ok = np.isfinite(disp) & (disp > 0)
        both = (got['disp'][:, 0] > 0) & ok
        assert both.sum() > 0.2 * ok.sum()
        rel = float(np.median(np.abs(got['disp'][:, 0][both].astype(np.float64) - disp[both]) / disp[both]))
        bound = voxel / float(np.median(fb / disp[both].astype(np.float64)))
        print(f'{p}: median |raycast - disp| / disp {rel:.3e}, a voxel of depth {bound:.3e}, hit {100 * (got["disp"] > 0).mean():.1f} %')
        assert rel <= bound
        ln = np.linalg.norm(got['normal'].astype(np.float64), axis=1)
        assert np.allclose(ln[got['disp'][:, 0] > 0], 1.0, atol=1e-5) and not ln[got['disp'][:, 0] == 0].any()
        hit += int((got['disp'] > 0).sum())
        pixels += got['disp'].size
    assert abs(hit / pixels - rep['hit']) < 1e-6
    assert _bytes(os.path.join(root, 'settings.npz')) == settings_before
    # a second run writes nothing; --force rewrites the same bytes
    stamp = {p: os.stat(os.path.join(p, 'raycast_gt.npz')).st_mtime_ns for p in paths}
    files = {p: _bytes(os.path.join(p, 'raycast_gt.npz')) for p in paths}
    assert RC.raycast_dataset(root, 'gt', res=RES) == 0
    assert all(os.stat(os.path.join(p, 'raycast_gt.npz')).st_mtime_ns == stamp[p] for p in paths)
    os.remove(os.path.join(paths[1], 'raycast_gt.npz'))
    assert RC.raycast_dataset(root, 'gt', res=RES) == 1
    RC.main([root, '--disp', 'gt', '--res', str(RES), '--force'])
    assert '2 raycast files written' in capsys.readouterr().out
    assert all(_bytes(os.path.join(p, 'raycast_gt.npz')) == files[p] for p in paths)
    assert all(sorted(os.listdir(p)) == ['flow.npz', 'frames.npz', 'raycast_gt.npz'] for p in paths)
    with pytest.raises(ValueError):
        RC.raycast_dataset(root, 'sgm')                                                    # no sgm_disp stored
    with pytest.raises(ValueError):
        RC.raycast_dataset(root, 'multi_frame')                                            # no multi_frame_disp.npz


def test_report_measures_an_estimate_against_the_ground_truth(tmp_path, capsys):
    """a stored estimate (the truth with 1 % noise) is measured against the ground truth before and after fusion; --step is honoured"""
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, raycast as RC
    from tests import fuse_inputs as FI
    shape = FI.SHAPES[3]
    n, tl, h, w = shape
    a = FI.make_input(shape, 'plane')
    root = str(tmp_path / 'plane')
    D.save_settings(root, synth.make_settings(h, w))
    d = os.path.join(root, '00000000')
    os.makedirs(d)
    b = a['batch']
    np.savez(os.path.join(d, 'frames.npz'), im=b['im0'][0], ambient=b['ambient0'][0], grad=np.zeros_like(b['im0'][0]), disp=b['disp0'][0],
             R=b['R'][0], t=b['t'][0])
    np.savez(os.path.join(d, 'single_frame_disp.npz'), disp=FI.make_input(shape, 'noise')['disp'][0][:, None])
    RC.main([root, '--disp', 'single_frame', '--res', '40', '--tol', '0.05', '--step', '0.5', '--report'])
    out = capsys.readouterr().out
    print(out)
    line = [l for l in out.split('\n') if l.startswith('raycast of the single_frame')][0]
    assert 'step 0.5 voxels' in line
    rep = _report_numbers(line)
    assert list(rep) == ['tracks', 'written', 'hit', 'kept', 'moved', 'err_in', 'err_out']
    assert rep['tracks'] == 1 and rep['written'] == 1 and rep['hit'] > 0 and rep['kept'] > 0 and rep['moved'] > 0
    assert np.isfinite(rep['err_in']) and rep['err_in'] > 0 and np.isfinite(rep['err_out']) and rep['err_out'] > 0
    assert sorted(os.listdir(d)) == ['frames.npz', 'raycast_single_frame.npz', 'single_frame_disp.npz']
    exact = RC.raycast_dataset(root, 'gt', res=40, report=True)
    assert 'err_in' not in exact and exact['hit'] > 0 and exact['moved'] < rep['moved']
