"""GPU, end to end: rendered tracks on disk, their poses and flows removed -> presave_pose --pairwise disp (ops.disp_align_poses on the
stored disparities, no flow) -> presave_flow --source geometry (ops.rigid_flow under those poses) -> frames.npz and flow.npz that a
multi-frame Worker trains from - against the flow-based chain (presave_flow on the ambient images, then presave_pose) on a copy.

Four tracks at 64 x 64, not two: the Worker's split sets one aside for testing and one for validation, and a step takes two."""
import argparse
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 64
N = 4


def _bytes(path):
    with open(path, 'rb') as fp:
        return fp.read()


def _arrays(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _strip(d):
    """frames.npz without R and t, no flow.npz -> (R, t, the flows) it held"""
    a = _arrays(os.path.join(d, 'frames.npz'))
    R, t = a.pop('R'), a.pop('t')
    np.savez(os.path.join(d, 'frames.npz'), **a)
    flows = _arrays(os.path.join(d, 'flow.npz'))
    os.remove(os.path.join(d, 'flow.npz'))
    return R, t, flows


def _errors(d, truth):
    """(mean rotation error of the pairs with frame 0 in rad, mean end-point error of the stored flows in px) against the rendered truth"""
    from depthinspace_amd.data import presave_pose as PP
    R, t, flows = truth
    a = _arrays(os.path.join(d, 'frames.npz'))
    tl = len(R)
    Rp, Rs = PP.relative_poses(R, t)[0], PP.relative_poses(a['R'], a['t'])[0]
    rot = float(np.mean([PP.rotation_angle(Rs[0, j] @ Rp[0, j].T) for j in range(1, tl)]))
    hit = a['disp'][:, 0] > 0
    got = _arrays(os.path.join(d, 'flow.npz'))
    epe = []
    for k, f in flows.items():
        e = np.sqrt(((got[k].astype(np.float64) - f) ** 2).sum(axis=1))[0]
        epe.append(e[hit[int(k[5])]].mean())
    return rot, float(np.mean(epe))


def test_disparity_chain_beats_the_flow_chain_and_feeds_a_worker(tmp_path, capsys):
    from depthinspace_amd.data import presave_flow as PF, presave_pose as PP, render
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    root, other = str(tmp_path / 'data'), str(tmp_path / 'flowchain')
    paths = render.write_rendered_dataset(root, st, N, seed=11)
    truth = [_strip(p) for p in paths]
    shutil.copytree(root, other)
    before = {p: _arrays(os.path.join(p, 'frames.npz')) for p in paths}
    settings_before = _bytes(os.path.join(root, 'settings.npz'))
    with pytest.raises(ValueError, match='flow.npz'):
        PP.presave_pose(root, 'gt')                                      # the flow-based stage has nothing to read
    with pytest.raises(ValueError, match='--joint reads flow.npz'):
        PP.presave_pose(root, 'gt', pairwise='disp', joint=True)         # and says so
    with pytest.raises(ValueError, match='stores no poses'):
        PF.presave_flow(root, source='geometry')
    capsys.readouterr()
    # 1. the disparity chain, by its command lines
    PP.main([root, '--pairwise', 'disp', '--disp', 'gt', '--report'])
    out = capsys.readouterr().out
    print(out)
    assert f'{N} tracks written' in out and 'failed and were left' not in out and 'aligned disparity maps' in out
    tl = len(truth[0][0])
    for p in paths:
        assert sorted(os.listdir(p)) == ['frames.npz']                   # no flow.npz was needed, no temporary file is left
    PF.main([root, '--source', 'geometry', '--disp', 'gt'])
    assert f'{N} tracks done' in capsys.readouterr().out
    keys = sorted(f'flow_{i}{j}' for i in range(tl) for j in range(tl) if i != j)
    for p in paths:
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz']
        after = _arrays(os.path.join(p, 'frames.npz'))
        assert sorted(after) == sorted(list(before[p]) + ['R', 't'])
        for k, v in before[p].items():
            assert after[k].dtype == v.dtype and after[k].shape == v.shape and after[k].tobytes() == v.tobytes(), k
        assert after['R'].dtype == np.float32 and after['R'].shape == (tl, 3, 3) and after['t'].shape == (tl, 3)
        assert np.array_equal(after['R'][0], np.eye(3)) and np.array_equal(after['t'][0], np.zeros(3))
        fl = _arrays(os.path.join(p, 'flow.npz'))
        assert sorted(fl) == keys and all(a.shape == (1, 2, H, W) and a.dtype == np.float32 and np.isfinite(a).all() for a in fl.values())
    assert _bytes(os.path.join(root, 'settings.npz')) == settings_before
    # 2. the flow-based chain on the copy
    assert PF.presave_flow(other) == N and PP.presave_pose(other, 'gt') == N
    figures = []
    for p, tr in zip(paths, truth):
        rot, epe = _errors(p, tr)
        rot_f, epe_f = _errors(os.path.join(other, os.path.basename(p)), tr)
        figures.append(f'{os.path.basename(p)}: rotation error {rot:.2e} rad (flow chain {rot_f:.2e}), end-point error {epe:.3f} px (flow chain {epe_f:.3f})')
        assert rot < rot_f and epe < epe_f
    # 3. a second run without --force changes nothing
    files = {p: (_bytes(os.path.join(p, 'frames.npz')), _bytes(os.path.join(p, 'flow.npz'))) for p in paths}
    stamps = {p: [os.stat(os.path.join(p, f)).st_mtime_ns for f in ('frames.npz', 'flow.npz')] for p in paths}
    assert PP.presave_pose(root, 'gt', pairwise='disp') == 0 and PF.presave_flow(root, source='geometry') == 0
    assert all([os.stat(os.path.join(p, f)).st_mtime_ns for f in ('frames.npz', 'flow.npz')] == stamps[p] for p in paths)
    assert all((_bytes(os.path.join(p, 'frames.npz')), _bytes(os.path.join(p, 'flow.npz'))) == files[p] for p in paths)
    # 4. --report: finite numbers, nothing written.  The stored flows are the chain's own, so the end-point error is that of a re-run.
    capsys.readouterr()
    rep = PP.presave_pose(root, 'gt', pairwise='disp', report=True)
    print(capsys.readouterr().out)
    assert rep['written'] == 0 and rep['tracks'] == N and rep['ok'] == N * tl * (tl - 1) and rep['failed'] == 0
    assert all(np.isfinite(rep[k]) for k in ('share', 'weight', 'resid', 'cycle_rot', 'cycle_trans', 'gt_rot', 'gt_trans'))
    PF.main([root, '--source', 'geometry', '--disp', 'gt', '--report'])
    line = capsys.readouterr().out
    print(line)
    res = PF.presave_flow(root, source='geometry', report=True)
    assert 'rigid flow of the gt disparities' in line and set(res) == {'epe', 'under0.5', 'under1', 'under2', 'visible', 'zeros'}
    assert all(np.isfinite(v) for v in res.values()) and res['epe'] == 0 and 0 < res['visible'] <= 1 and 0 <= res['zeros'] < 1
    assert all((_bytes(os.path.join(p, 'frames.npz')), _bytes(os.path.join(p, 'flow.npz'))) == files[p] for p in paths)
    # 5. a multi-frame Worker takes a step from the root (any stored disparity will do as the primary one here)
    for p in paths:
        with np.load(os.path.join(p, 'frames.npz')) as f:
            np.savez(os.path.join(p, 'single_frame_disp.npz'), disp=f['disp'])
    args = argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic', architecture='multi_frame',
                              epochs=1, warmup_epochs=150, train_batch_size=2, max_disp=128)
    out_dir = str(tmp_path / 'out')
    w = multi_frame_worker.Worker(args, data_root=root, output_dir=out_dir, num_workers=0, test_batch_size=1)
    assert len(w.train_paths) == 2
    torch.manual_seed(2)
    net = multi_frame_networks.FuseNet(imsize=w.imsizes[0], K=w.K, baseline=w.baseline, track_length=4, max_disp=128).cuda()
    opt = FlatAdam(net.parameters(), lr=1e-4)
    p0 = opt.flat_p.clone()
    w.do(net, opt, cmd='retrain')
    assert opt.step_count == 1 and not torch.equal(p0, opt.flat_p) and bool(torch.isfinite(opt.flat_p).all())
    m = json.load(open(os.path.join(out_dir, 'multi_frame', 'metrics.json')))
    assert np.all(np.isfinite(m['0']['train']['loss']))
    print('\n'.join(figures))                                      # (capsys holds what was printed before its last read)
