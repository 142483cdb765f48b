"""GPU, end to end at 64 x 64: rendered mesh-scene tracks written to disk (packed) -> DIS-SF and DIS-MF training through
Worker(data_root=...), as tests/test_pipeline_gpu.py does on synth's tracks; and render_batch handed straight to copy_data."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _args(arch, epochs, bs=2):
    return argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic', architecture=arch,
                              epochs=epochs, warmup_epochs=150, train_batch_size=bs, max_disp=128)


def test_rendered_tracks_train_sf_and_mf(tmp_path):
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, packed, render
    from depthinspace_amd.model import networks, multi_frame_networks, single_frame_worker, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    H = W = 64
    settings = synth.make_settings(H, W)
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, settings, 6, seed=3, pack=True)
    assert len(paths) == 6 and sorted(os.listdir(paths[5])) == ['flow.f32', 'flow.npz', 'frames.f32', 'frames.npz']
    with np.load(os.path.join(paths[0], 'frames.npz')) as f:
        disp = f['disp']
        assert disp.shape == (4, 1, H, W) and np.isfinite(disp).all() and disp.min() > 0   # the board fills every view
        assert np.isfinite(f['im']).all() and 0 <= f['im'].min() and f['im'].max() <= 1
    # depth discontinuities: somewhere in the six tracks neighbouring pixels differ by more than a pixel of disparity
    jump = max(float(np.abs(np.diff(np.load(os.path.join(p, 'frames.npz'))['disp'], axis=-1)).max()) for p in paths)
    assert jump > 1.0, jump
    out = str(tmp_path / 'out')
    mk = dict(data_root=root, output_dir=out, num_workers=2, test_batch_size=1)
    # ---- DIS-SF: one epoch = 4 training tracks / bs 2 = two steps, through the packed loader
    w = single_frame_worker.Worker(_args('single_frame', 1), **mk)
    assert len(w.train_paths) == 4 and os.path.exists(os.path.join(root, 'packed.json'))
    torch.manual_seed(1)
    net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
    opt = FlatAdam(net.parameters(), lr=1e-4)
    p0 = opt.flat_p.clone()
    w.do(net, opt, cmd='retrain')
    assert opt.step_count == 2 and not torch.equal(p0, opt.flat_p) and bool(torch.isfinite(opt.flat_p).all())
    m = json.load(open(os.path.join(out, 'single_frame', 'metrics.json')))
    assert np.all(np.isfinite(m['0']['train']['loss'])) and np.all(np.isfinite(m['0']['test']['0']['loss']))
    # ---- DIS-MF on stored single-frame disparities (any stored disparity will do here: the rendered one), packed again
    for p in paths:
        with np.load(os.path.join(p, 'frames.npz')) as f:
            np.savez(os.path.join(p, 'single_frame_disp.npz'), disp=f['disp'])
    assert len(packed.pack_dataset(root)) == 6
    wm = multi_frame_worker.Worker(_args('multi_frame', 1), **mk)
    torch.manual_seed(2)
    netm = multi_frame_networks.FuseNet(imsize=wm.imsizes[0], K=wm.K, baseline=wm.baseline, track_length=4, max_disp=128).cuda()
    optm = FlatAdam(netm.parameters(), lr=1e-4)
    p0 = optm.flat_p.clone()
    wm.do(netm, optm, cmd='retrain')
    assert optm.step_count == 2 and not torch.equal(p0, optm.flat_p) and bool(torch.isfinite(optm.flat_p).all())
    m = json.load(open(os.path.join(out, 'multi_frame', 'metrics.json')))
    assert np.all(np.isfinite(m['0']['train']['loss']))


def test_render_batch_equals_tracks_read_back(tmp_path):
    """render_batch -> copy_data gives the first-step loss of the same tracks written to disk and read back (frames in file order)"""
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D, render
    from depthinspace_amd.model import networks, single_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    H = W = 64
    settings = synth.make_settings(H, W)
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, settings, 2, seed=21)
    ds = D.TrackNpzDataset(root, paths, track_length=4, train=False, load_flow_data=True)
    disk = D.collate([ds[0], ds[1]])
    direct = render.render_batch(settings, 2, 4, seed=21)
    assert set(direct) == set(disk) and all(v.is_cuda for v in direct.values())
    for k in disk:
        assert tuple(direct[k].shape) == tuple(disk[k].shape), k
        assert torch.equal(direct[k].cpu(), disk[k]), k
    losses = []
    for batch in (direct, disk):
        w = single_frame_worker.Worker(_args('single_frame', 1), settings=settings)
        w.build_losses()
        torch.manual_seed(4)
        net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
        errs, _ = w.train_step(net, FlatAdam(net.parameters(), lr=1e-4), batch)
        torch.cuda.synchronize()
        losses.append([float(e.detach()) for e in errs])
    # (the same bits go in; the loss sums are fp64 atomics, so the last bit of a term may depend on arrival order)
    assert np.isfinite(losses[0]).all() and np.allclose(losses[0], losses[1], rtol=1e-6, atol=0), losses
