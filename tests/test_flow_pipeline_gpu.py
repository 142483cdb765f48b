"""GPU, end to end at 64 x 64 (the size the other pipeline tests train at): tracks on disk without a flow.npz ->
data/presave_flow.py (ops.dense_flow on the stored ambient frames) -> pack -> a multi-frame Worker reads them and trains."""
import argparse
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 64


def _bytes(path):
    with open(path, 'rb') as fp:
        return fp.read()


def _root(tmp_path, n=6):
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D
    root = str(tmp_path / 'data')
    paths = D.write_synthetic_dataset(root, synth.make_settings(H, W), n, seed=50)
    return root, paths


def test_presave_writes_the_flows_of_dense_flow_and_nothing_else(tmp_path, capsys):
    from depthinspace_amd import ops
    from depthinspace_amd.data import presave_flow as P
    root, paths = _root(tmp_path, 3)
    exact = str(tmp_path / 'exact')
    shutil.copytree(root, exact)
    for p in paths:
        os.remove(os.path.join(p, 'flow.npz'))
    before = {p: _bytes(os.path.join(p, 'frames.npz')) for p in paths}
    settings_before = _bytes(os.path.join(root, 'settings.npz'))
    assert P.presave_flow(root) == 3
    keys = sorted(f'flow_{i}{j}' for i in range(4) for j in range(4) if i != j)
    stored = {}
    for p in paths:
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz']           # no temporary file is left
        with np.load(os.path.join(p, 'frames.npz')) as f:
            amb = torch.from_numpy(f['ambient']).cuda()
        want = ops.dense_flow(amb[None, :, 0]).cpu().numpy()
        with np.load(os.path.join(p, 'flow.npz')) as f:
            assert sorted(f.files) == keys
            for i in range(4):
                for j in range(4):
                    if i != j:
                        a = f[f'flow_{i}{j}']
                        assert a.shape == (1, 2, H, W) and a.dtype == np.float32
                        assert np.array_equal(a, want[:, i * 4 + j]), (p, i, j)
        assert _bytes(os.path.join(p, 'frames.npz')) == before[p]
        stored[p] = want
    assert _bytes(os.path.join(root, 'settings.npz')) == settings_before
    # incremental: nothing left to do, nothing rewritten; a missing one alone is redone; --force redoes all, with other parameters
    assert P.presave_flow(root) == 0
    os.remove(os.path.join(paths[1], 'flow.npz'))
    assert P.presave_flow(root) == 1
    with np.load(os.path.join(paths[1], 'flow.npz')) as f:
        assert sorted(f.files) == keys and np.array_equal(f['flow_10'], stored[paths[1]][:, 4])
    assert P.presave_flow(root, iters=13, force=True) == 3
    with np.load(os.path.join(paths[0], 'flow.npz')) as f, np.load(os.path.join(paths[0], 'frames.npz')) as g:
        want = ops.dense_flow(torch.from_numpy(g['ambient']).cuda()[None, :, 0], iters=13).cpu().numpy()
        assert np.array_equal(f['flow_23'], want[:, 11]) and not np.array_equal(want, stored[paths[0]])
    # the command line; --report on the root that kept its exact flows: finite numbers, nothing written
    P.main([root, '--force', '--iters', '13', '--warps', '1'])
    assert '3 tracks done' in capsys.readouterr().out
    listing = {p: sorted(os.listdir(os.path.join(exact, p))) for p in sorted(os.listdir(exact)) if os.path.isdir(os.path.join(exact, p))}
    flows = {p: _bytes(os.path.join(exact, p, 'flow.npz')) for p in listing}
    res = P.presave_flow(exact, report=True)
    line = capsys.readouterr().out
    print(line)
    assert 'epe' in line and set(res) == {'epe', 'under0.5', 'under1', 'under2'}
    assert all(np.isfinite(v) for v in res.values()) and 0 <= res['under0.5'] <= res['under1'] <= res['under2'] <= 1
    assert listing == {p: sorted(os.listdir(os.path.join(exact, p))) for p in listing}
    assert all(_bytes(os.path.join(exact, p, 'flow.npz')) == flows[p] for p in listing)
    os.remove(os.path.join(paths[2], 'flow.npz'))
    with pytest.raises(ValueError):
        P.presave_flow(root, report=True)                                     # nothing to compare with


def test_a_multi_frame_worker_trains_on_the_presaved_flows(tmp_path):
    from depthinspace_amd.data import presave_flow as P
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    root, paths = _root(tmp_path, 6)
    for p in paths:
        os.remove(os.path.join(p, 'flow.npz'))
        with np.load(os.path.join(p, 'frames.npz')) as f:                    # any stored disparity will do as the primary one here
            np.savez(os.path.join(p, 'single_frame_disp.npz'), disp=f['disp'])
    assert P.presave_flow(root, pack=True) == 6
    assert os.path.exists(os.path.join(root, 'packed.json')) and all(os.path.exists(os.path.join(p, 'flow.f32')) for p in paths)
    args = argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic', architecture='multi_frame',
                              epochs=1, warmup_epochs=150, train_batch_size=2, max_disp=128)
    out = str(tmp_path / 'out')
    w = multi_frame_worker.Worker(args, data_root=root, output_dir=out, num_workers=2, test_batch_size=1)
    torch.manual_seed(2)
    net = multi_frame_networks.FuseNet(imsize=w.imsizes[0], K=w.K, baseline=w.baseline, track_length=4, max_disp=128).cuda()
    opt = FlatAdam(net.parameters(), lr=1e-4)
    p0 = opt.flat_p.clone()
    w.do(net, opt, cmd='retrain')
    assert opt.step_count == 2 and not torch.equal(p0, opt.flat_p) and bool(torch.isfinite(opt.flat_p).all())
    m = json.load(open(os.path.join(out, 'multi_frame', 'metrics.json')))
    assert np.all(np.isfinite(m['0']['train']['loss']))
