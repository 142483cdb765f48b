"""GPU, end to end: rendered tracks on disk -> python -m depthinspace_amd.data.raycast --disp gt -> a DIS-SF worker that reads
raycast_gt.npz as its pseudo ground truth (--pseudo_gt_source raycast_gt --pseudo_gt_erode 1), from the .npz tracks and, after
python -m depthinspace_amd.data.packed, from the packed root: the same planes, the same four masked terms.

DispNetS takes 64 x 48 (widths 48, 24, 12, 6, 3, 2, 1, 1 with crop_like), so the size of tests/test_raycast_pipeline_gpu.py is kept.
Seen on the MI355X at --res 48, seed 11: 84.2 % of the pixels of the two tracks have a surface, 68.0 % are left at erode 1."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import masked_l1_ref as R

H, W, RES = 64, 48, 48
ERODE = 1


def _args():
    return argparse.Namespace(use_pseudo_gt=True, lcn_radius=5, track_length=4, data_type='synthetic', architecture='single_frame',
                              epochs=1, warmup_epochs=150, train_batch_size=2, max_disp=128, pseudo_gt_source='raycast_gt',
                              pseudo_gt_erode=ERODE)


def _listing(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def _first_test_batch(root, paths):
    """an SF worker on `root` and the first batch of both tracks in test-mode order (frames 0 .. 3, no augmentation)"""
    from depthinspace_amd.model import single_frame_worker
    w = single_frame_worker.Worker(_args(), data_root=root, num_workers=0, test_batch_size=2)
    w.build_losses()
    w.current_epoch = 2
    dset = w._make_dataset(paths, False, True, 0, 0)
    assert dset.pseudo_stem == 'raycast_gt'
    return w, next(iter(w._loader(dset, 2, False, 0)))


def _pseudo_terms(w, net, batch):
    """-> (pseudo_gt as the worker holds it, the weighted terms, the four estimates), numpy"""
    w.copy_data(batch, device=w.train_device, requires_grad=False, train=False)
    flow = w.read_optical_flow(False)
    with torch.no_grad():
        out = w.net_forward(net, flow)
        errs = w.loss_forward(out, False, flow)
    torch.cuda.synchronize()
    assert len(out) == 4 and len(errs) == 15
    return (w.data['pseudo_gt'].cpu().numpy(), np.array([e.cpu().numpy() for e in errs], dtype=np.float32),
            [o.cpu().numpy() for o in out])


def _check_terms(terms, outs, target):
    vals, _, n = R.masked_l1_multi(outs, target, ERODE)
    assert 0 < n < target.size
    for s in range(4):
        want = np.float32(vals[s] * np.float32(0.1 / 2 ** s))
        # (value within one float32 ulp of the restatement on real-valued data, then one rounding of the weighted product)
        assert abs(float(terms[11 + s]) - float(want)) <= 2.0 * 2.0 ** -23 * float(want), (s, terms[11 + s], want)


def test_sf_worker_trains_on_raycast_pseudo_gt(tmp_path, capsys):
    from depthinspace_amd.data import packed as P, raycast as RC, render
    from depthinspace_amd.model import networks
    from depthinspace_amd.trainer import FlatAdam
    from tests import render_scenes
    st = render_scenes.small_settings(H, W)
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    RC.main([root, '--disp', 'gt', '--res', str(RES)])
    assert '2 raycast files written' in capsys.readouterr().out
    files = [np.load(os.path.join(p, 'raycast_gt.npz'))['disp'] for p in paths]

    w, batch = _first_test_batch(root, paths)
    assert isinstance(batch, dict)                                           # the DataLoader(TrackNpzDataset) path
    torch.manual_seed(3)
    net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
    net.train()
    pg, terms, outs = _pseudo_terms(w, net, batch)
    # pseudo_gt is the file, (tl, bs, 1, H, W); it has holes and it is not empty
    assert pg.shape == (4, 2, 1, H, W) and pg.dtype == np.float32
    assert all(np.array_equal(pg[:, b], files[b]) for b in range(2))
    share = float((pg > 0).mean())
    print(f'valid share of raycast_gt at --res {RES}: {share:.3f}; eroded by {ERODE}: {R.valid_mask(pg, ERODE).mean():.3f}')
    assert 0.2 <= share < 1
    _check_terms(terms, outs, pg)

    # the packed root: the same planes, the same terms; nothing but .f32 files and packed.json is added
    before = _listing(root)
    written = P.pack_dataset(root)
    assert sorted(os.path.basename(f) for f in written) == sorted(['flow.f32', 'frames.f32', 'raycast_gt.f32'] * 2)
    assert sorted(set(_listing(root)) - set(before)) == sorted(['packed.json'] + [os.path.relpath(f, root) for f in written])
    wp, pbatch = _first_test_batch(root, paths)
    assert isinstance(pbatch, P.PackedBatch) and pbatch.loader.pseudo_stem == 'raycast_gt'
    pg_p, terms_p, outs_p = _pseudo_terms(wp, net, pbatch)
    assert pg_p.tobytes() == pg.tobytes()
    _check_terms(terms_p, outs_p, pg_p)
    np.testing.assert_allclose(terms_p, terms, rtol=1e-6, atol=0)            # same inputs: run-to-run noise only

    # one training step on that batch leaves finite parameters
    opt = FlatAdam(net.parameters(), lr=1e-4)
    p0 = opt.flat_p.clone()
    errs, _ = w.train_step(net, opt, batch)
    torch.cuda.synchronize()
    assert len(errs) == 15 and all(bool(torch.isfinite(e)) for e in errs)
    assert bool(torch.isfinite(opt.flat_p).all()) and not torch.equal(opt.flat_p, p0)
