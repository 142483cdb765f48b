"""GPU: dis_assemble_tracks against the numpy reference (tests/packed_ref.py), and the packed loader through Worker.copy_data, one
eager DIS-MF step and the real training / test loops (`do('retrain')`, graph and eager) against the .npz path on the same tracks."""
import argparse
import itertools
import json
import os
import shutil

import numpy as np
import pytest
import torch

from depthinspace_amd.data import packed as P
from tests import packed_ref as R

pytestmark = pytest.mark.gpu


def _args(arch, epochs=1, bs=2, pgt=False):
    return argparse.Namespace(use_pseudo_gt=pgt, lcn_radius=5, track_length=4, data_type='synthetic', architecture=arch,
                              epochs=epochs, warmup_epochs=150, train_batch_size=bs, max_disp=128)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _check_kernel(bs, tl, h, w, perm, has_sgm=False, primary=False, pseudo=False, want_sgm=None, pad=0, misalign=False, seed=0):
    from depthinspace_amd import ops
    size = P.record_layout(h, w, has_sgm, primary, pseudo)['size']
    stride = size + pad
    rng = np.random.RandomState(seed)
    raw = rng.standard_normal(bs * stride + 1).astype(np.float32)
    dev = torch.from_numpy(raw).cuda()
    # misalign: the records start 4 bytes into a 16-byte aligned allocation
    host, draw = (raw[1:], dev[1:]) if misalign else (raw[:-1], dev[:-1])
    assert draw.data_ptr() % 16 == (4 if misalign else 0)
    perm = np.asarray(perm, np.int32).reshape(bs, tl)
    ref = R.assemble(host, stride, perm, h, w, has_sgm, primary, pseudo, want_sgm)
    shapes = {k: v.shape for k, v in ref.items()}
    out = {k: torch.full(s, float('nan'), device='cuda') for k, s in shapes.items()}
    got = ops.assemble_tracks(draw, torch.from_numpy(perm).cuda(), bs, tl, h, w, has_sgm=has_sgm, primary=primary, pseudo=pseudo,
                              want_sgm=want_sgm, record_stride=stride, out=out)
    torch.cuda.synchronize()
    assert isinstance(got, P.AssembledBatch) and set(got) == set(ref), set(got) ^ set(ref)
    for k, v in ref.items():
        assert got[k] is out[k]
        assert torch.equal(got[k].cpu(), torch.from_numpy(v)), k      # (NaN anywhere: an element that was not written)
    fs = got['_flow_stacked']
    for i in range(tl):
        assert not bool(fs[i * tl + i].any()), 'diagonal flow planes are exactly zero'
    fresh = ops.assemble_tracks(draw, torch.from_numpy(perm).cuda(), bs, tl, h, w, has_sgm=has_sgm, primary=primary, pseudo=pseudo,
                                want_sgm=want_sgm, record_stride=stride)
    assert all(torch.equal(fresh[k], got[k]) and tuple(fresh[k].shape) == shapes[k] for k in ref)


def test_kernel_small_and_scalar_path():
    _check_kernel(1, 2, 8, 12, [[2, 0]])
    _check_kernel(3, 3, 31, 33, [[3, 1, 0], [0, 1, 2], [2, 3, 1]], primary=True)        # h * w = 1023: the 4-byte path
    _check_kernel(3, 3, 31, 33, [[1, 2, 3], [3, 2, 1], [0, 3, 2]], has_sgm=True, primary=True, pseudo=True)


def test_kernel_every_frame_order():
    orders = list(itertools.permutations(range(4)))
    assert len(orders) == 24
    for c in range(12):
        _check_kernel(2, 4, 64, 64, [orders[2 * c], orders[2 * c + 1]], primary=True, seed=c)


@pytest.mark.parametrize('has_sgm,primary,pseudo,want_sgm', [(False, False, False, None), (True, False, False, None),
                                                             (True, True, True, None), (True, True, False, False),
                                                             (False, False, True, None), (False, True, True, None)])
def test_kernel_optional_fields(has_sgm, primary, pseudo, want_sgm):
    _check_kernel(2, 4, 16, 20, [[3, 0, 2, 1], [1, 2, 3, 0]], has_sgm, primary, pseudo, want_sgm)
    _check_kernel(2, 3, 16, 20, [[3, 0, 2], [1, 2, 0]], has_sgm, primary, pseudo, want_sgm)


def test_kernel_stride_and_alignment_fallback():
    perm = [[1, 3, 0, 2], [2, 0, 3, 1]]
    _check_kernel(2, 4, 64, 64, perm, primary=True, pad=8)                    # a stride larger than the record, still 16-byte
    _check_kernel(2, 4, 64, 64, perm, primary=True, pad=3)                    # record 1 is not 16-byte aligned
    _check_kernel(2, 4, 64, 64, perm, primary=True, misalign=True)            # h * w % 4 == 0, raw 4 bytes off
    _check_kernel(5, 4, 64, 72, [list(np.random.RandomState(b).permutation(4)) for b in range(5)], has_sgm=True, primary=True,
                  pseudo=True)                                                 # more than one tile per plane, many blocks
    # 448 planes x 5 tiles: more tiles than the capped grid has blocks, so the grid-stride loop takes a second round
    _check_kernel(8, 4, 128, 136, [list(np.random.RandomState(40 + b).permutation(4)) for b in range(8)], has_sgm=True, primary=True,
                  pseudo=True)


def test_kernel_masks_the_table():
    """entries outside 0..3 are masked, equal entries give zero flow planes: no table content reads outside a record"""
    from depthinspace_amd import ops
    h, w, bs, tl = 16, 20, 1, 4
    size = P.record_layout(h, w)['size']
    raw = torch.randn(size, device='cuda')
    bad = torch.tensor([[7, 1 << 20, -1, 2]], dtype=torch.int32, device='cuda')      # & 3 -> 3 0 3 2
    got = ops.assemble_tracks(raw, bad, bs, tl, h, w)
    ref = R.assemble(raw.cpu().numpy(), size, [[3, 0, 1, 2]], h, w, False, False, False)   # (slot 2 differs: checked apart)
    for i in (0, 1, 3):
        assert torch.equal(got['im0'][i].cpu(), torch.from_numpy(ref['im0'][i]))
    assert torch.equal(got['im0'][2], got['im0'][0])
    assert not bool(got['_flow_stacked'][0 * tl + 2].any()) and not bool(got['_flow_stacked'][2 * tl + 0].any())
    assert torch.equal(got['_flow_stacked'][1 * tl + 3].cpu(), torch.from_numpy(ref['_flow_stacked'][1 * tl + 3]))


# ------------------------------------------------------------------------------------------------ roots shared by the rest
@pytest.fixture(scope='module')
def roots(tmp_path_factory):
    """an 8-track 64x64 root with the DIS-SF disparities, and a packed copy of it"""
    base = tmp_path_factory.mktemp('packed_gpu')
    npz, packed = str(base / 'npz'), str(base / 'packed')
    R.make_root(npz, 64, 64, 8, seed=60, pseudo=False)
    shutil.copytree(npz, packed)
    P.pack_dataset(packed)
    return npz, packed


def _mf_worker(root, bs, **kw):
    from depthinspace_amd.model import multi_frame_worker
    w = multi_frame_worker.Worker(_args('multi_frame', bs=bs), data_root=root, num_workers=0, test_batch_size=1, **kw)
    w.device_aug = False     # (the augmentation draws are host-RNG driven: off, so that both paths see the same batches)
    return w


def _both_batches(roots, bs, seed):
    """the same tracks in the same frame orders: a collated .npz batch and the packed loader's first batch"""
    from depthinspace_amd.data.dataset import collate
    npz, packed = roots
    wn, wp = _mf_worker(npz, bs), _mf_worker(packed, bs)
    order = [5, 2, 7][:bs]
    ds = wn.get_train_set()
    ds.sample_paths = sorted(os.path.join(npz, d) for d in os.listdir(npz) if d.startswith('0'))
    np.random.seed(seed)
    batch = collate([ds[i] for i in order])
    dp = wp.get_train_set()
    dp.sample_paths = sorted(os.path.join(packed, d) for d in os.listdir(packed) if d.startswith('0'))
    ld = P.loader_for(dp, order, bs, True, 2, seed, wp.train_device, packed)
    return wn, batch, wp, next(iter(ld)), ld


def test_copy_data_equals_npz_path(roots):
    wn, batch, wp, pb, ld = _both_batches(roots, 2, 31)
    assert pb.raw.is_cuda and pb.perm.is_cuda and not pb.released
    wn.copy_data(batch, device=wn.train_device, requires_grad=False, train=True)
    wp.copy_data(pb, device=wp.train_device, requires_grad=False, train=True)
    assert pb.released
    torch.cuda.synchronize()
    assert set(wp.data) == set(wn.data) | {'_flow_stacked'}
    for k, v in wn.data.items():
        assert wp.data[k].shape == v.shape and torch.equal(wp.data[k], v), k
    assert wp.data['im0'].shape == (4, 2, 2, 64, 64) and wp.data['std0'].shape == (4, 2, 1, 64, 64)
    fo = wp.read_optical_flow(train=True)
    assert fo.stacked is wp.data['_flow_stacked'] and fo['flow_31'].data_ptr() == fo.stacked[3 * 4 + 1].data_ptr()


def test_eager_mf_step_equals_npz_path(roots):
    """inputs bit-identical, so only the run-to-run noise of tests/test_determinism_gpu.py remains: loss terms to rtol 1e-6, the
    flat gradient to 1e-5 of its largest entry"""
    from depthinspace_amd.model import multi_frame_networks
    from depthinspace_amd.trainer import FlatAdam
    wn, batch, wp, pb, ld = _both_batches(roots, 1, 17)
    torch.manual_seed(0)
    net = multi_frame_networks.FuseNet(wn.imsizes[0], wn.K, wn.baseline).cuda()
    opt = FlatAdam(net.parameters(), lr=1e-4)
    runs = []
    for w, data in ((wn, batch), (wp, pb)):
        w.build_losses()
        w.current_epoch = 2
        w.copy_data(data, device=w.train_device, requires_grad=False, train=True)
        opt.zero_grad()
        flow = w.read_optical_flow(True)
        out = w.net_forward(net, flow)
        losses = w.loss_forward(out, True, flow)
        sum(losses).backward()
        torch.cuda.synchronize()
        runs.append((np.array([float(l) for l in losses]), opt.flat_g.clone()))
    (l0, g0), (l1, g1) = runs
    gmax = float(g0.abs().max())
    worst = float((g1 - g0).abs().max()) / gmax
    print('packed vs npz step: losses', l0, l1, 'max gradient difference / max |gradient| =', worst)
    np.testing.assert_allclose(l1, l0, rtol=1e-6, atol=0)
    assert gmax > 0 and worst < 1e-5


@pytest.mark.parametrize('arch', ['single_frame', 'multi_frame'])
def test_retrain_on_packed_root_graph_equals_eager(roots, tmp_path, arch):
    from depthinspace_amd.model import networks, multi_frame_networks, single_frame_worker, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    npz, packed = roots
    mod = multi_frame_worker if arch == 'multi_frame' else single_frame_worker

    def make_net(w):
        torch.manual_seed(5)
        if arch == 'multi_frame':
            return multi_frame_networks.FuseNet(imsize=w.imsizes[0], K=w.K, baseline=w.baseline, track_length=4, max_disp=128).cuda()
        return networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
    res = {}
    for mode in ('eager', 'graph'):
        out = str(tmp_path / ('out_' + mode))
        w = mod.Worker(_args(arch), data_root=packed, output_dir=out, num_workers=0, test_batch_size=1, use_graph=(mode == 'graph'))
        w.device_aug = False
        net = make_net(w)
        opt = FlatAdam(net.parameters(), lr=1e-4)
        w.do(net, opt, cmd='retrain')
        m = json.load(open(os.path.join(out, arch, 'metrics.json')))
        assert w.last_epoch_stats['steps'] == 3 and w.last_epoch_stats['step_mode'] == mode      # 6 train tracks / bs 2
        assert w.last_epoch_stats['frames_per_s'] > 0
        res[mode] = (opt.flat_p.clone(), m['0']['train']['loss'], opt.step_count, w, net)
    assert res['eager'][2] == res['graph'][2] == 3
    # the bounds of tests/test_pipeline_gpu.py::test_worker_train_epoch_graph_equals_eager
    d = (res['eager'][0] - res['graph'][0]).abs()
    assert float(d.max()) <= 2.1e-4 * res['eager'][2] and float(d.mean()) < 2e-6
    np.testing.assert_allclose(res['graph'][1], res['eager'][1], rtol=5e-3, atol=1e-5)
    # test_epoch: the packed root against the unpacked copy, same network; 3 tracks in batches of 2 (a smaller last batch)
    wp, net = res['eager'][3], res['eager'][4]
    wu = mod.Worker(_args(arch), data_root=npz, output_dir=str(tmp_path / 'out_npz'), num_workers=0, test_batch_size=2)
    wp.test_batch_size = 2
    got = {}
    for name, w in (('packed', wp), ('npz', wu)):
        w.build_losses()
        dset = w._make_dataset(w.train_paths[:3], False, False, 0, 0)
        loader = w._loader(dset, 2, False, 0)
        assert isinstance(loader, P.PackedTrackLoader) == (name == 'packed') and len(loader) == 2
        loss = w.test_epoch(0, 0, net, dset)
        got[name] = (loss, dict(w.metric_data['0']['test']['0']))
    np.testing.assert_allclose(got['packed'][0], got['npz'][0], rtol=1e-6, atol=0)
    assert set(got['packed'][1]) == set(got['npz'][1]) and 'dist2_mean' in got['npz'][1]
    for k, v in got['npz'][1].items():
        np.testing.assert_allclose(got['packed'][1][k], v, rtol=1e-6, atol=0, err_msg=k)
