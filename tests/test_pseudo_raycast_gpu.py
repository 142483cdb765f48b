"""GPU: the DIS-SF worker on a pseudo ground truth with holes (--pseudo_gt_source raycast_*, --pseudo_gt_erode): the four masked
terms against the numpy restatement tests/masked_l1_ref.py next to the untouched photometric / smoothness / geometric terms, the
step eagerly and through trainer.GraphedStep, and the default path (multi_frame, erode 0), which must stay the four ops.l1_mean
terms bit for bit."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import masked_l1_ref as R

H = W = 64
WEIGHTS = [np.float32(0.1 / 2 ** s) for s in range(4)]


def make_args(bs, use_pseudo_gt, data_type='synthetic', **new):
    """tests/test_sf_gpu.py's make_args, plus the two new fields where a test gives them"""
    return argparse.Namespace(use_pseudo_gt=use_pseudo_gt, lcn_radius=5, track_length=4, data_type=data_type,
                              architecture='single_frame', epochs=1, warmup_epochs=150, train_batch_size=bs,
                              max_disp=128, **new)


def _setup(holes=True):
    from depthinspace_amd import synth
    settings = synth.make_settings(H, W)
    batch = synth.make_batch(settings, 1, 4, seed=77, with_pseudo_gt=True)
    pg = np.array(batch['pseudo_gt'], dtype=np.float32, copy=True)            # (bs, tl, 1, H, W)
    assert pg.shape == (1, 4, 1, H, W) and (pg > 0).all()
    if holes:                                                                 # rectangles, one at a border, one frame untouched
        pg[0, 0, 0, 10:22, 5:30] = 0
        pg[0, 1, 0, 0:7, 50:64] = 0
        pg[0, 1, 0, 40, 41] = 0
        pg[0, 3, 0, 30:64, 0:9] = 0
    batch['pseudo_gt'] = pg
    return settings, {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}


def _worker(settings, **kw):
    from depthinspace_amd.model import single_frame_worker
    w = single_frame_worker.Worker(make_args(1, **kw), settings=settings)
    w.build_losses()
    w.current_epoch = 2
    return w


def _net_and_opt(w):
    from depthinspace_amd.model import networks
    from depthinspace_amd.trainer import FlatAdam
    torch.manual_seed(0)
    net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
    return net, FlatAdam(net.parameters(), lr=1e-4)


def _forward_backward(w, net, opt, batch):
    """the body of Worker.train_step without the optimiser step -> (weighted terms: float32 array, the four estimates)"""
    w.copy_data(batch, device=w.train_device, requires_grad=False, train=True)
    opt.zero_grad()
    flow = w.read_optical_flow(True)
    out = w.net_forward(net, flow)
    errs = w.loss_forward(out, True, flow)
    errs.total.backward()
    torch.cuda.synchronize()
    return np.array([e.detach().cpu().numpy() for e in errs], dtype=np.float32), [o.detach().cpu().numpy() for o in out]


def test_terms_are_the_other_terms_plus_the_restatement():
    settings, batch = _setup()
    w_off = _worker(settings, use_pseudo_gt=False)
    w_on = _worker(settings, use_pseudo_gt=True, pseudo_gt_source='raycast_gt', pseudo_gt_erode=1)
    net, opt = _net_and_opt(w_on)
    base, _ = _forward_backward(w_off, net, opt, batch)
    g_off = opt.flat_g.clone()
    got, outs = _forward_backward(w_on, net, opt, batch)
    assert len(outs) == 4 and len(got) == len(base) + 4 and len(base) == 4 + 1 + 6
    # photometric + smooth + geometric: the same launches on the same inputs (run-to-run noise of their fp64 atomic sums only)
    np.testing.assert_allclose(got[:len(base)], base, rtol=1e-6, atol=0)
    # the four masked terms: value (within one float32 ulp of the restatement on real-valued data) times its weight (one rounding)
    target = w_on.data['pseudo_gt'].cpu().numpy()                             # (tl, bs, 1, H, W), as the term reads it
    assert np.array_equal(target, np.swapaxes(batch['pseudo_gt'].numpy(), 0, 1))
    vals, _, n = R.masked_l1_multi(outs, target, 1)
    assert 0 < n < target.size
    for s in range(4):
        want = np.float32(vals[s] * WEIGHTS[s])
        print(s, got[len(base) + s], want)
        assert abs(float(got[len(base) + s]) - float(want)) <= 2.0 * 2.0 ** -23 * float(want), (s, got[len(base) + s], want)
    assert torch.isfinite(opt.flat_g).all() and not torch.equal(opt.flat_g, g_off)


def test_graphed_step_matches_eager():
    """one FlatAdam step eagerly and the same step through trainer.GraphedStep, under the bounds of
    tests/test_dp_gpu.py::test_graphed_step_matches_eager"""
    from depthinspace_amd.trainer import GraphedStep
    settings, batch = _setup()
    w = _worker(settings, use_pseudo_gt=True, pseudo_gt_source='raycast_gt', pseudo_gt_erode=1)
    net, opt = _net_and_opt(w)
    state = (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.state_dev)
    snap = [t.clone() for t in state]
    eager = GraphedStep(w, net, opt, batch, use_graph=False)
    eager.run()
    torch.cuda.synchronize()
    p_eager, l_eager = opt.flat_p.clone(), eager.losses()
    assert opt.step_count == 1 and len(l_eager) == 15 and not torch.equal(p_eager, snap[0])
    graphed = GraphedStep(w, net, opt, batch, use_graph=True, warmup=1, strict=True)
    graphed.run()   # eager warm-up step + capture + first replay
    torch.cuda.synchronize()
    assert graphed.mode == 'graph'
    for t, c in zip(state, snap):
        t.copy_(c)
    graphed.run()
    torch.cuda.synchronize()
    assert opt.step_count == 1
    assert float((opt.flat_p - p_eager).abs().max()) < 2.5e-4
    assert float((opt.flat_p - p_eager).abs().mean()) < 2e-6
    np.testing.assert_allclose(graphed.losses(), l_eager, rtol=2e-3, atol=1e-5)
    assert bool(torch.isfinite(opt.flat_p).all())


def test_default_path_is_untouched():
    """pseudo_gt_source='multi_frame', erode 0 and a hole-free target: the terms of a Namespace without the new fields, bit for bit"""
    settings, batch = _setup(holes=False)
    w_old = _worker(settings, use_pseudo_gt=True)
    w_new = _worker(settings, use_pseudo_gt=True, pseudo_gt_source='multi_frame', pseudo_gt_erode=0)
    assert not hasattr(make_args(1, True), 'pseudo_gt_source')
    net, opt = _net_and_opt(w_old)
    a, _ = _forward_backward(w_old, net, opt, batch)
    ga = opt.flat_g.clone()
    b, outs = _forward_backward(w_new, net, opt, batch)
    assert len(a) == len(b) == 15 and a.tobytes() == b.tobytes()
    # ... and they are ops.l1_mean's: mean |o - t| over every pixel
    t = w_new.data['pseudo_gt'].cpu().numpy().astype(np.float64)
    for s in range(4):
        want = np.abs(outs[s].astype(np.float64) - t).mean() * 0.1 / 2 ** s
        assert abs(float(b[11 + s]) - want) <= 1e-6 * want
    assert float((opt.flat_g - ga).abs().max()) <= 1e-5 * float(ga.abs().max())
