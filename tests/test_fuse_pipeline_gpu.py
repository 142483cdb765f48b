"""GPU, end to end: rendered tracks on disk -> python -m depthinspace_amd.data.fuse (ops.fuse_track on the stored disparities and poses)
-> one PLY per track, and the consistency report."""
import os

import numpy as np
import pytest
import torch

from tests import fuse_inputs as FI

pytestmark = pytest.mark.gpu

H, W, TOL = 64, 48, 0.01


def _bytes(path):
    with open(path, 'rb') as fp:
        return fp.read()


def _report_numbers(line):
    tok = line.split(': ', 1)[1].split()
    return {tok[k]: float(tok[k + 1]) for k in range(0, len(tok) - 1, 2)}


def test_fuse_command_on_rendered_tracks(tmp_path, capsys):
    from depthinspace_amd import ops
    from depthinspace_amd.data import dataset as D, fuse as F, ply, render
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    before = {p: {f: _bytes(os.path.join(p, f)) for f in os.listdir(p)} for p in paths}
    settings_before = _bytes(os.path.join(root, 'settings.npz'))
    capsys.readouterr()
    F.main([root, '--disp', 'gt', '--report'])
    out = capsys.readouterr().out
    print(out)
    assert '2 clouds written' in out
    rep = _report_numbers([l for l in out.split('\n') if l.startswith('fusion of the gt')][0])
    assert set(rep) == {'valid', 'seen', 'consistent', 'resid', 'points', 'tracks', 'written'}     # gt against itself: no gt_distance
    assert rep['tracks'] == 2 and rep['written'] == 2 and 0 < rep['valid'] <= 1 and 0 < rep['seen'] <= 1
    assert 0.5 < rep['consistent'] <= 1 and 0 <= rep['resid'] and rep['points'] > 0            # occlusion keeps it below 1 here
    K = st.K.astype(np.float64)
    points = 0
    for p in paths:
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz', 'fused_gt.ply']      # no temporary file is left
        for f, b in before[p].items():
            assert _bytes(os.path.join(p, f)) == b, f
        rec, comments = ply.read_ply(os.path.join(p, 'fused_gt.ply'))
        assert rec.dtype == ply.VERTEX_DTYPE and len(comments) == 1 and 'gt' in comments[0]
        with np.load(os.path.join(p, 'frames.npz')) as f:
            disp, R, t, amb = f['disp'][:, 0], f['R'], f['t'], f['ambient'][:, 0]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)[None]).cuda()
        r = ops.fuse_track(up(disp), up(R), up(t), st.K, st.baseline, up(amb), tol=TOL, min_views=2, want_dense=True)
        count = int(r['count'].sum().item())
        assert len(rec) == count > 0
        points += count
        xyz = np.stack([rec['x'], rec['y'], rec['z']], 1)
        src = r['src'][:count].cpu().numpy().astype(np.int64)
        assert np.array_equal(xyz, r['xyz'][:count].cpu().numpy()) and np.array_equal(rec['intensity'], amb.reshape(-1)[src])
        views = r['views'][0].cpu().numpy().reshape(-1)[src]
        assert np.array_equal(rec['views'], views) and views.min() >= 2
        nrm = np.stack([rec['nx'], rec['ny'], rec['nz']], 1)
        ln = np.linalg.norm(nrm, axis=1)
        assert np.all((ln == 0) | (np.abs(ln - 1) < 1e-5)) and (ln > 0).any()
        # every point lies within tol max_j |X_j| of the ground-truth point of its pixel: each averaged sample sits on camera j's ray
        # within tol X_j.z in depth, that is within tol |X_j| of the point
        Xw, z = F.gt_points(disp, R, t, st, src)
        frame = src // (H * W)
        Xj = np.einsum('jab,mb->jma', R.astype(np.float64), Xw) + t.astype(np.float64)[:, None]
        far = np.linalg.norm(Xj, axis=2)
        far[frame, np.arange(len(src))] = 0                                             # j != i
        dist = np.linalg.norm(xyz.astype(np.float64) - Xw, axis=1)
        print(f'{p}: {count} points, max distance / bound {np.max(dist / (TOL * far.max(0))):.4f}')
        assert np.all(dist <= TOL * far.max(0))
    assert points == rep['points'] and _bytes(os.path.join(root, 'settings.npz')) == settings_before
    # a second run writes nothing; --force rewrites the same bytes
    stamp = {p: os.stat(os.path.join(p, 'fused_gt.ply')).st_mtime_ns for p in paths}
    clouds = {p: _bytes(os.path.join(p, 'fused_gt.ply')) for p in paths}
    assert F.fuse_dataset(root, 'gt') == 0
    assert all(os.stat(os.path.join(p, 'fused_gt.ply')).st_mtime_ns == stamp[p] for p in paths)
    os.remove(os.path.join(paths[1], 'fused_gt.ply'))
    assert F.fuse_dataset(root, 'gt') == 1
    F.main([root, '--disp', 'gt', '--force'])
    assert '2 clouds written' in capsys.readouterr().out
    assert all(_bytes(os.path.join(p, 'fused_gt.ply')) == clouds[p] for p in paths)
    with pytest.raises(ValueError):
        F.fuse_dataset(root, 'sgm')                                                       # no sgm_disp stored
    with pytest.raises(ValueError):
        F.fuse_dataset(root, 'multi_frame')                                               # no multi_frame_disp.npz


def test_report_on_exact_and_on_perturbed_disparities(tmp_path, capsys):
    """a plane without occluders: every seen pair of exact disparities is consistent, up to the pairs float32 may decide either way;
    a stored estimate (here: the truth with 1 % noise) is also measured against the ground truth"""
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, fuse as F
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
    rep = F.fuse_dataset(root, 'gt', tol=TOL, report=True)
    r32, r64, ex, ex_pairs = FI.refs(shape, 'plane', 0)
    seen_pairs = int(r64['seen_ij'].sum())
    print(capsys.readouterr().out, f'exempt pairs {int(ex_pairs.sum())} of {seen_pairs} seen')
    assert rep['tracks'] == 1 and rep['written'] == 1 and rep['valid'] == 1.0 and 'gt_distance' not in rep
    assert 1.0 - ex_pairs.sum() / seen_pairs <= rep['consistent'] <= 1.0
    assert abs(rep['seen'] - seen_pairs / FI.pair_count(shape)) <= ex_pairs.sum() / FI.pair_count(shape)
    noisy = F.fuse_dataset(root, 'single_frame', tol=TOL, report=True)
    print(capsys.readouterr().out)
    assert sorted(os.listdir(d)) == ['frames.npz', 'fused_gt.ply', 'fused_single_frame.ply', 'single_frame_disp.npz']
    assert noisy['consistent'] < rep['consistent'] and noisy['resid'] > rep['resid']
    # 1 % multiplicative noise on the disparity is 1 % on the depth; averaging agreeing views can only bring a point closer
    assert 0 < noisy['gt_distance'] < 0.03
