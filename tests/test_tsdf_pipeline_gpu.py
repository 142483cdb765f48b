"""GPU, end to end: rendered tracks on disk -> python -m depthinspace_amd.data.mesh (ops.fuse_track for the placement,
ops.tsdf_integrate and ops.tsdf_mesh on the stored disparities and poses) -> one triangle mesh per track, and the report."""
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


def test_mesh_command_on_rendered_tracks(tmp_path, capsys):
    from depthinspace_amd import ops
    from depthinspace_amd.data import mesh as M, ply, render
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    before = {p: {f: _bytes(os.path.join(p, f)) for f in os.listdir(p)} for p in paths}
    settings_before = _bytes(os.path.join(root, 'settings.npz'))
    capsys.readouterr()
    M.main([root, '--disp', 'gt', '--res', str(RES), '--report'])
    out = capsys.readouterr().out
    print(out)
    assert '2 meshes written' in out
    rep = _report_numbers([l for l in out.split('\n') if l.startswith('meshes of the gt')][0])
    assert set(rep) == {'tracks', 'written', 'vertices', 'triangles', 'observed', 'boundary', 'area'}   # gt against itself: no gt term
    assert rep['tracks'] == 2 and rep['written'] == 2 and rep['triangles'] > 0 and rep['vertices'] > 0
    assert 0 < rep['observed'] < 1 and 0 <= rep['boundary'] < 1.5 and rep['area'] > 0
    vertices = triangles = 0
    area = 0.0
    for p in paths:
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz', 'mesh_gt.ply']        # no temporary file is left
        for f, b in before[p].items():
            assert _bytes(os.path.join(p, f)) == b, f
        rec, faces, comments = ply.read_mesh(os.path.join(p, 'mesh_gt.ply'))
        assert rec.dtype == ply.VERTEX_DTYPE and len(comments) == 1 and 'gt' in comments[0]
        with np.load(os.path.join(p, 'frames.npz')) as f:
            disp, R, t, amb = f['disp'][:, 0], f['R'], f['t'], f['ambient'][:, 0]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        # a direct call with the same placement
        r = ops.fuse_track(up(disp)[None], up(R)[None], up(t)[None], st.K, st.baseline, up(amb)[None], tol=0.01, min_views=2)
        m = int(r['count'].sum().item())
        assert m > 0
        origin, voxel, trunc, grid = M.place_volume(r['xyz'][:m], RES, None, 3.0)
        assert max(grid) in (RES, RES + 1) and min(grid) >= 2 and abs(trunc - 3 * voxel) <= 1e-6 * trunc
        lo = r['xyz'][:m].min(dim=0).values.cpu().numpy()
        assert np.all(origin <= lo - 3.99 * voxel) and np.all(origin >= lo - 4.01 * voxel)
        vol = ops.tsdf_integrate(up(disp), up(R), up(t), st.K, st.baseline, up(amb), origin=origin, voxel=voxel, trunc=trunc, grid=grid)
        g = ops.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel)
        nv, nf = (int(v) for v in g['count'].tolist())
        assert len(rec) == nv > 0 and len(faces) == nf > 0
        xyz = np.stack([rec['x'], rec['y'], rec['z']], 1)
        assert np.array_equal(xyz, g['xyz'].cpu().numpy()) and np.array_equal(faces, g['faces'].cpu().numpy())
        assert np.array_equal(np.stack([rec['nx'], rec['ny'], rec['nz']], 1), g['normal'].cpu().numpy())
        assert np.array_equal(rec['intensity'], g['value'].cpu().numpy()) and np.array_equal(rec['views'], g['views'].cpu().numpy())
        assert rec['views'].min() >= 1 and rec['views'].max() <= disp.shape[0]
        vertices += nv
        triangles += nf
        area += M.mesh_stats(xyz, faces)[1]
    assert vertices == rep['vertices'] and triangles == rep['triangles'] and abs(area - rep['area']) <= 1e-5 * area
    assert _bytes(os.path.join(root, 'settings.npz')) == settings_before
    # a second run writes nothing; --force rewrites the same bytes
    stamp = {p: os.stat(os.path.join(p, 'mesh_gt.ply')).st_mtime_ns for p in paths}
    meshes = {p: _bytes(os.path.join(p, 'mesh_gt.ply')) for p in paths}
    assert M.mesh_dataset(root, 'gt', res=RES) == 0
    assert all(os.stat(os.path.join(p, 'mesh_gt.ply')).st_mtime_ns == stamp[p] for p in paths)
    os.remove(os.path.join(paths[1], 'mesh_gt.ply'))
    assert M.mesh_dataset(root, 'gt', res=RES) == 1
    M.main([root, '--disp', 'gt', '--res', str(RES), '--force'])
    assert '2 meshes written' in capsys.readouterr().out
    assert all(_bytes(os.path.join(p, 'mesh_gt.ply')) == meshes[p] for p in paths)
    assert all(sorted(os.listdir(p)) == ['flow.npz', 'frames.npz', 'mesh_gt.ply'] for p in paths)
    with pytest.raises(ValueError):
        M.mesh_dataset(root, 'sgm')                                                        # no sgm_disp stored
    with pytest.raises(ValueError):
        M.mesh_dataset(root, 'multi_frame')                                                # no multi_frame_disp.npz


def test_report_measures_an_estimate_against_the_ground_truth(tmp_path, capsys):
    """a stored estimate (the truth with 1 % noise) is also measured against the ground truth; --voxel and --min-weight are honoured"""
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, mesh as M, ply
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
    exact = M.mesh_dataset(root, 'gt', res=40, report=True)
    noisy = M.mesh_dataset(root, 'single_frame', res=40, tol=0.05, report=True)
    print(capsys.readouterr().out)
    assert sorted(os.listdir(d)) == ['frames.npz', 'mesh_gt.ply', 'mesh_single_frame.ply', 'single_frame_disp.npz']
    assert 'gt_depth_error' not in exact and exact['triangles'] > 0 and noisy['triangles'] > 0
    rec, faces, comments = ply.read_mesh(os.path.join(d, 'mesh_gt.ply'))
    voxel = float(comments[0].split('voxel ')[1].split(',')[0])
    xyz = np.stack([rec['x'], rec['y'], rec['z']], 1)
    gt = b['disp0'][0][:, 0]
    st = D.load_settings(root)
    # a plane without occluders: the mesh lies on the ground truth it was made from, within a voxel in depth at every projection
    s, k = M.gt_depth_error(xyz, gt, b['R'][0], b['t'][0], st)
    zmin = float((xyz @ b['R'][0][0].T + b['t'][0][0])[:, 2].min())
    assert k >= len(xyz) and zmin > 0 and s / k < voxel / zmin
    # 1 % multiplicative noise on the disparity is 1 % on the depth; the volume averages the frames, a voxel is allowed on top
    assert 0 < noisy['gt_depth_error'] < 0.01 + voxel / zmin
    M.main([root, '--disp', 'gt', '--voxel', f'{voxel:g}', '--min-weight', str(tl), '--force', '--report'])
    out = capsys.readouterr().out
    strict = _report_numbers([l for l in out.split('\n') if l.startswith('meshes of the gt')][0])
    assert 0 < strict['triangles'] <= exact['triangles'] and strict['written'] == 1
    rec2, _, comments2 = ply.read_mesh(os.path.join(d, 'mesh_gt.ply'))
    assert rec2['views'].min() == tl and f'min_weight {tl}' in comments2[0] and f'voxel {voxel:g}' in comments2[0]
