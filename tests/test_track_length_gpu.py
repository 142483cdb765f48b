"""DIS-MF at track lengths 2 and 3 on the HIP path: the parameter-free geometry and Conv3D's neighbour sets bit for bit, the
Conv3D kernels (select, forward, the class-ordered / float-atomic / CSR backward forms) and the 64 / 96-channel 1 x 1 conv_mf
against restatements, and the free-running training step against the reference's own step at tl = 2 / 3
(tests/golden/mf_*_tl{2,3}_*.npz, scripts/make_golden_track_length.py)."""
import argparse
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import dis_oracle as O

TLS = [2, 3]
MF_TL_GOLDENS = ['mf_64_tl2_bs1', 'mf_64_tl3_bs2_rnd', 'mf_128_tl3_bs1']


def relerr(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _stack_flows(flow, tl, bs, h, w):
    fl = torch.zeros(tl * tl, bs, 2, h, w)
    for i in range(tl):
        for j in range(tl):
            if i != j:
                fl[i * tl + j] = flow[f'flow_{i}{j}']
    return fl


def _select_tl(wxyz, wmask, stride, tl):
    """tests/bitexact.py's Conv3D selection over 9 tl candidates: ids (tl,bs,ho,wo,9) in torch.topk's order"""
    from tests import bitexact as B
    assert wxyz.shape[1] == tl
    return B.conv3d_select(wxyz, wmask, stride)


@pytest.mark.parametrize('tl', TLS)
@pytest.mark.parametrize('cfg', [(64, 48, 2, 8, True, {}), (128, 128, 1, 4321, False, dict(scene='bumps', motion=1.5))])
def test_mf_geometry_masks_and_selection_bit_exact_at_track_length(tl, cfg):
    """tests/test_net_ops_gpu.py::test_mf_geometry_masks_and_selection_bit_exact at tl slots: core / quarter geometry, the fb
    masks and both neighbour sets of the HIP path equal tests/bitexact.py bit for bit; the slot weights follow the masks."""
    from depthinspace_amd import ops, synth, lib
    from tests import bitexact as B
    H, W, bs, seed, rnd, kw = cfg
    st = synth.make_settings(H, W)
    b = synth.make_random_batch(st, bs, tl, seed=seed) if rnd else synth.make_batch(st, bs, tl, seed=seed, **kw)
    tb = {k: torch.from_numpy(v).transpose(0, 1).contiguous() if v.ndim > 2 else torch.from_numpy(v) for k, v in b.items()}
    h, w = H // 2, W // 2
    eq = np.array_equal
    depth = ops.disp_to_depth(tb['primary_disp'].cuda(), float(st.K[0, 0]) * st.baseline)
    e_depth = B.disp_to_depth(tb['primary_disp'].numpy(), float(st.K[0, 0]), st.baseline)
    assert eq(depth.cpu().numpy(), e_depth)
    depth_core = ops.resize_planar(depth.view(tl, bs, H, W), (h, w), True)
    e_dc = B.resize_ac(e_depth, h, w)
    assert eq(depth_core.cpu().numpy(), e_dc[:, :, 0])
    flow = {k: v[0] for k, v in tb.items() if k.startswith('flow_')}
    assert len(flow) == tl * (tl - 1)
    ff = _stack_flows(flow, tl, bs, H, W).cuda()
    fc_p = ops.resize_planar(ff, (h, w), True, flow_scale=(float(w) / float(W), float(h) / float(H)))
    e_fc = {k: B.resize_flow(v.numpy(), h, w) for k, v in flow.items()}
    fl = ops.planar_to_nhwc(fc_p.view(tl * tl * bs, 2, h, w)).view(tl * tl, bs, h, w, 2)
    Ki = lib.host_floats(np.linalg.inv(st.K).reshape(-1))
    geom = ops.mf_geometry(depth_core, tb['R'].cuda(), tb['t'].cuda(), fl, Ki, W // w, H // h)
    assert tuple(geom.shape) == (tl, bs, h, w, tl, 4)
    ex, em = B.mf_geometry(e_dc, O.mf_core_rays(st.K, H, W).numpy(), tb['R'].numpy(), tb['t'].numpy(), e_fc)
    assert eq(geom[..., 3].permute(0, 4, 1, 2, 3).unsqueeze(3).cpu().numpy(), em)
    assert eq(geom[..., :3].permute(0, 4, 1, 5, 2, 3).cpu().numpy(), ex)
    hq, wq = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    gq = ops.mf_geometry_resize(geom, (hq, wq))
    exq = B.resize_ac(ex, hq, wq)
    emq = (B.resize_ac(em, hq, wq) > 0.5).astype(np.float32)
    assert eq(gq[..., :3].permute(0, 4, 1, 5, 2, 3).cpu().numpy(), exq)
    assert eq(gq[..., 3].permute(0, 4, 1, 2, 3).unsqueeze(3).cpu().numpy(), emq)
    # Conv3D neighbour sets over 9 tl candidates: torch.topk's ids in torch.topk's order
    idx = ops.conv3d_select(geom, 2)
    idx_q = ops.conv3d_select(gq, 1)
    assert int(idx.max()) < 9 * tl and int(idx_q.max()) < 9 * tl
    assert eq(idx.cpu().numpy(), _select_tl(ex, em, 2, tl))
    assert eq(idx_q.cpu().numpy(), _select_tl(exq, emq, 1, tl))
    # slot weighting mask / mean(mask) over the tl slots
    wm = torch.from_numpy(em)
    ref = wm / wm.mean(dim=1, keepdim=True)   # (tl,slot,bs,1,h,w)
    sw = ops.slot_weights(geom)               # (tl*bs,h,w,slot)
    assert relerr(sw.view(tl, bs, h, w, tl).permute(0, 4, 1, 2, 3), ref[:, :, :, 0]) < 1e-6


def _conv3d_inputs(tl, seed, bs=2, h=12, w=14):
    """a per-target geometry (tl,bs,h,w,tl,4) with distinct slots, masks with holes, and features (tl,bs,h,w,tl,32)"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(tl, tl, bs, 3, h, w, generator=g) * 0.05
    xyz[:, :, :, 2] += 3.0
    uu, vv = O.pixel_grid(h, w)
    xyz[:, :, :, 0] += (uu - w / 2) * 0.01
    xyz[:, :, :, 1] += (vv - h / 2) * 0.01
    mask = (torch.rand(tl, tl, bs, 1, h, w, generator=g) > 0.2).float()
    mask[:, 0] = 1
    feat = torch.randn(tl, tl, bs, 32, h, w, generator=g)
    geom = torch.cat([xyz, mask], dim=3).permute(0, 2, 4, 5, 1, 3).contiguous()   # (tl,bs,h,w,slot,4)
    wf = feat.permute(0, 2, 4, 5, 1, 3).contiguous()                             # (tl,bs,h,w,slot,32)
    return xyz, mask, feat, geom, wf, g


@pytest.mark.parametrize('tl', TLS)
@pytest.mark.parametrize('stride', [1, 2])
def test_conv3d_matches_oracle_at_track_length(tl, stride):
    """Conv3D (ops.conv3d_select + ops.conv3d_knn + GroupNorm, the default class-ordered backward) at tl slots against the oracle's
    conv3d_knn(tl=) run on the same neighbour sets (which equal tests/bitexact.py's, in order), with test_conv3d_golden's bars."""
    from depthinspace_amd import ops
    xyz, mask, feat, geom, wf, g = _conv3d_inputs(tl, 40 + 10 * tl + stride)
    bs, C, h, w = feat.shape[2:]
    name = 'blocks.0.conv3d_1'
    p = O.init_params({k: v for k, v in O.mf_param_shapes(tl=tl).items() if k.startswith(name)}, seed=5)
    pd = {k[len(name) + 1:]: v.detach().cuda().requires_grad_(True) for k, v in p.items()}
    geom_d = geom.cuda()
    wf_d = wf.cuda().requires_grad_(True)
    idx = ops.conv3d_select(geom_d, stride)
    ho, wo = idx.shape[2:4]
    assert np.array_equal(idx.cpu().numpy(), _select_tl(xyz.numpy(), mask.numpy(), stride, tl))
    y = ops.conv3d_knn(geom_d, wf_d, pd['dense1.0.weight'], pd['dense1.0.bias'], pd['dense2.0.weight'], pd['dense2.0.bias'],
                       pd['w'], idx, stride)
    out = ops.group_norm(y.view(tl * bs, ho, wo, C), pd['bn.weight'], pd['bn.bias']).view(tl, bs, ho, wo, C)
    go = torch.randn(tl, bs, ho, wo, C, generator=g)
    out.backward(go.cuda())
    # the oracle, every target on the HIP path's neighbour sets
    O.CONV3D_FORCE = {'core' if stride == 2 else 'quarter': idx.long().cpu()}
    try:
        fo = feat.clone().requires_grad_(True)
        ys = [O.conv3d_knn(p, name, xyz[ti], fo[ti], mask[ti], stride, tl, target=ti) for ti in range(tl)]
    finally:
        O.CONV3D_FORCE = None
    yo = torch.stack(ys, 0)   # (tl,bs,C,ho,wo)
    yo.backward(go.permute(0, 1, 4, 2, 3))
    assert relerr(out.permute(0, 1, 4, 2, 3), yo) < 2e-5
    assert relerr(wf_d.grad.permute(0, 4, 1, 5, 2, 3), fo.grad) < 5e-5
    for k_ in ('w', 'dense1.0.weight', 'dense1.0.bias', 'dense2.0.weight', 'dense2.0.bias', 'bn.weight', 'bn.bias'):
        assert relerr(pd[k_].grad, p[f'{name}.{k_}'].grad) < 1e-4, k_


@pytest.mark.parametrize('tl', TLS)
@pytest.mark.parametrize('stride', [1, 2])
def test_conv3d_class_ordered_backward_at_track_length(tl, stride):
    """At tl slots: the class-ordered backward (dis_conv3d_knn_bwd_det) equals round 1-2's float-atomic kernel to rounding and
    repeats bit for bit."""
    from depthinspace_amd import ops
    _, _, _, geom, _, g = _conv3d_inputs(tl, 70 + 10 * tl + stride)
    _, bs, h, w, _, _ = geom.shape
    C = 32
    name = 'blocks.0.conv3d_1'
    p = O.init_params({k: v for k, v in O.mf_param_shapes(tl=tl).items() if k.startswith(name)}, seed=6)
    pd = {k[len(name) + 1:]: v.detach().cuda() for k, v in p.items()}
    geom = geom.cuda()
    wf = torch.randn(tl, bs, h, w, tl, C, generator=g).cuda()
    idx = ops.conv3d_select(geom, stride)
    ho, wo = idx.shape[2:4]
    y, agg, y0 = [torch.empty((tl, bs, ho, wo, C), device='cuda') for _ in range(3)]
    args = (geom, wf, pd['dense1.0.weight'], pd['dense1.0.bias'], pd['dense2.0.weight'], pd['dense2.0.bias'], pd['w'], idx)
    ops.lib.call('dis_conv3d_knn_fwd_agg', *args, y, agg, tl, bs, h, w, stride)
    ops.lib.call('dis_conv3d_knn_fwd', *args, y0, tl, bs, h, w, stride)
    assert torch.equal(y, y0)
    gy = torch.randn(y.shape, generator=g).cuda()
    base = torch.randn(wf.shape, generator=g).cuda()
    acc = torch.empty(ops.lib.fn('dis_conv3d_knn_bwd_workspace')(), device='cuda')
    accd = torch.empty(ops.lib.fn('dis_conv3d_knn_bwd_det_workspace')(tl, bs, h, w, stride), device='cuda')
    g_at, gp_at = base.clone(), torch.empty(1632, device='cuda')
    ops.lib.call('dis_conv3d_knn_bwd', *args, y, gy, g_at, gp_at, acc, tl, bs, h, w, stride)
    scale = float((g_at - base).abs().max())
    assert scale > 0
    det = []
    for rep in range(2):
        g_d, gp_d = base.clone(), torch.empty(1632, device='cuda')
        ops.lib.call('dis_conv3d_knn_bwd_det', *args, y, agg, gy, g_d, gp_d, accd, tl, bs, h, w, stride)
        det.append((g_d, gp_d))
    assert float((det[0][0] - g_at).abs().max()) < 2e-6 * scale
    assert relerr(det[0][1], gp_at) < 2e-6
    assert torch.equal(det[0][0], det[1][0]) and torch.equal(det[0][1], det[1][1])   # bitwise reproducible


@pytest.mark.parametrize('tl', [1, 5, 8])
def test_conv3d_rejects_other_track_lengths(tl):
    """only the instanced track lengths are accepted: everything else is refused before a launch"""
    from depthinspace_amd import ops, lib
    geom = torch.zeros(tl, 1, 8, 8, tl, 4, device='cuda')
    idx = torch.zeros(tl, 1, 4, 4, 9, dtype=torch.uint8, device='cuda')
    assert lib.fn('dis_conv3d_knn_select')(geom.data_ptr(), idx.data_ptr(), tl, 1, 8, 8, 2, None) == -2   # DIS_ERR_UNSUPPORTED
    assert lib.fn('dis_conv3d_knn_bwd_det_workspace')(tl, 1, 8, 8, 2) == -1
    with pytest.raises(lib.DisHipError):
        ops.conv3d_select(geom, 2)


@pytest.mark.parametrize('cin', [64, 96])
@pytest.mark.parametrize('n,h,w', [(3, 19, 23), (2, 32, 48)])
def test_conv1x1_scaled_input_at_track_length(cin, n, h, w):
    """ops.conv2d_scaled_in for conv_mf at tl = 2 / 3 (Conv2d(32 tl, 32, 1) over the mask-weighted slots): output, statistics,
    input gradient (the scaled 32 -> cin input-gradient kernel), weight and bias gradient against an fp64 torch restatement, with
    the bars of the 128-channel case; then behind a GroupNorm, whose backward reaches this conv as a plain gradient (the lazy
    GroupNorm 1 x 1 form is 128 / 32 only)."""
    from depthinspace_amd import ops
    ns = cin // 32
    g = torch.Generator().manual_seed(n * 100 + h + cin)
    x = torch.randn(n, h, w, cin, generator=g)
    sc = torch.rand(n, h, w, ns, generator=g) * 2
    wt = torch.randn(32, cin, 1, 1, generator=g) / cin ** 0.5
    b = torch.randn(32, generator=g) * 0.1
    go = torch.randn(n, h, w, 32, generator=g)
    xr, wr, br = [v.double().requires_grad_(True) for v in (x, wt, b)]
    xs = (xr.view(n, h, w, ns, 32) * sc.double().unsqueeze(-1)).view(n, h, w, cin)
    yr = F.conv2d(xs.permute(0, 3, 1, 2), wr, br).permute(0, 2, 3, 1)
    yr.backward(go.double())
    xd, wd, bd = x.cuda().requires_grad_(True), wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    yd, st = ops.conv2d_scaled_in(xd, sc.cuda(), wd, bd, 1, 0, want_stats=True)
    yd.backward(go.cuda())
    assert relerr(yd, yr) < 2e-6
    s_ref = torch.stack([yr.sum(dim=(1, 2, 3)), (yr ** 2).sum(dim=(1, 2, 3))], dim=1).reshape(-1)
    assert torch.allclose(st.cpu().double(), s_ref.detach(), rtol=1e-6, atol=1e-4)
    assert relerr(xd.grad, xr.grad) < 5e-6
    assert relerr(wd.grad, wr.grad) < 5e-6
    assert relerr(bd.grad, br.grad) < 5e-6
    # conv_mf -> GroupNorm(1 group), as in Block2D3D
    gam, bet = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1
    xr2, wr2 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    xs2 = (xr2.view(n, h, w, ns, 32) * sc.double().unsqueeze(-1)).view(n, h, w, cin)
    o = F.conv2d(xs2.permute(0, 3, 1, 2), wr2, b.double())
    mr = F.group_norm(o, 1, gam.double(), bet.double(), eps=1e-5).permute(0, 2, 3, 1)
    mr.backward(go.double())
    xd2, wd2 = x.cuda().requires_grad_(True), wt.cuda().requires_grad_(True)
    o_d, st_d = ops.conv2d_scaled_in(xd2, sc.cuda(), wd2, b.cuda(), 1, 0, want_stats=True)
    md = ops.group_norm(o_d, gam.cuda(), bet.cuda(), stats=st_d)
    md.backward(go.cuda())
    assert relerr(md, mr) < 1e-5
    assert relerr(xd2.grad, xr2.grad) < 5e-5
    assert relerr(wd2.grad, wr2.grad) < 5e-5


def _args(bs, tl):
    return argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=tl, data_type='synthetic',
                              architecture='multi_frame', epochs=1, warmup_epochs=150, train_batch_size=bs, max_disp=128)


def _golden_batch(G):
    from depthinspace_amd import synth
    tl, H, W, bs = int(G['tl']), int(G['H']), int(G['W']), int(G['bs'])
    settings = synth.make_settings(H, W)
    mk = synth.make_random_batch if int(G['random_batch']) else synth.make_batch
    return settings, mk(settings, bs, tl, seed=int(G['bseed']))


@pytest.mark.parametrize('name', MF_TL_GOLDENS)
def test_mf_step_matches_reference_at_track_length(golden_dir, name):
    """FREE-RUNNING DIS-MF step at tl = 2 / 3 against the reference's own step (FuseNet(track_length=tl)), with the bars of
    tests/test_step_gpu.py::test_mf_step_matches_reference: ids, disparity, loss terms, gradients, Adam."""
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    G = np.load(os.path.join(golden_dir, name + '.npz'))
    tl, H, W, bs = int(G['tl']), int(G['H']), int(G['W']), int(G['bs'])
    settings, batch = _golden_batch(G)
    params = O.init_params(O.mf_param_shapes(tl=tl), seed=int(G['pseed']))
    net = multi_frame_networks.FuseNet(imsize=(H, W), K=settings.K, baseline=settings.baseline, track_length=tl, max_disp=128)
    net.load_state_dict({k: v.detach() for k, v in params.items()})
    net = net.cuda()
    w = multi_frame_worker.Worker(_args(bs, tl), settings=settings)
    w.build_losses()
    w.current_epoch = int(G['epoch'])
    opt = FlatAdam(net.parameters(), lr=1e-4)
    errs, out = w.train_step(net, opt, {k: torch.from_numpy(v) for k, v in batch.items()})
    torch.cuda.synchronize()
    assert net.knn_index_override is None and tuple(out.shape) == (tl, bs, 1, H, W)
    assert np.array_equal(net.last_knn_index[0].cpu().numpy(), G['knn_idx_core'])
    assert np.array_equal(net.last_knn_index[1].cpu().numpy(), G['knn_idx_quarter'])
    ref_out = torch.from_numpy(G['out0'])
    l1 = float((out.detach().cpu() - ref_out).abs().mean())
    mx = float((out.detach().cpu() - ref_out).abs().max())
    assert l1 < 1e-4 and mx < 2e-3, (l1, mx)
    vals = np.array([float(e.detach()) for e in errs])
    assert len(vals) == len(G['vals'])
    np.testing.assert_allclose(vals, G['vals'], rtol=2e-4, atol=2e-6)
    named = dict(net.named_parameters())
    keys = list(G['grad_keys'])
    for i, k in enumerate(keys):
        g = named[k].grad
        if bool(G['grad_none'][i]):
            assert float(g.abs().max()) == 0.0, k
            continue
        l2_ref = float(G['grad_l2'][i])
        assert abs(float(g.double().norm()) - l2_ref) <= 2e-3 * l2_ref + 1e-12, (k, float(g.double().norm()), l2_ref)
        if 'grad:' + k in G.files:
            err = float((g.cpu() - torch.from_numpy(G['grad:' + k])).abs().max()) / (float(G['grad_absmax'][i]) + 1e-20)
            assert err < 2e-3, (k, err)
    checked = 0
    for k in keys:
        if 'new:' + k in G.files:
            d = (named[k].detach().cpu() - torch.from_numpy(G['new:' + k])).abs()
            g_ref = torch.from_numpy(G['grad:' + k]).abs()
            sure = g_ref > max(1e-3 * float(g_ref.max()), 1e-6)
            checked += int(sure.sum())
            if bool(sure.any()):
                assert float(d[sure].max()) <= 1e-6, (k, float(d[sure].max()))
            assert float(d.max()) <= 2.1e-4, k
    assert checked > 1000, checked
    print(name, 'disp L1', l1, 'max', mx, 'post-Adam entries checked to 1e-6:', checked)


def test_graphed_step_matches_eager_at_track_length_3():
    """trainer.GraphedStep at tl = 3: two replays of the captured step land on the parameters of two eager steps from the same
    state (no hidden tl = 4 in the capture, the flat buffers or the feature warp's untiled path: 24 threads per pixel do not
    divide 256)."""
    from depthinspace_amd import synth
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam, GraphedStep
    H = W = 64
    tl = 3
    settings = synth.make_settings(H, W)
    torch.manual_seed(0)
    w = multi_frame_worker.Worker(_args(1, tl), settings=settings)
    net = multi_frame_networks.FuseNet((H, W), settings.K, settings.baseline, track_length=tl).cuda()
    w.build_losses()
    w.current_epoch = 2
    opt = FlatAdam(net.parameters(), lr=1e-4)
    batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(settings, 1, tl, seed=77).items()}
    state = (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.state_dev)
    snap = [t.clone() for t in state]
    eager = GraphedStep(w, net, opt, batch, use_graph=False)
    for _ in range(2):
        eager.run()
    torch.cuda.synchronize()
    p_eager, l_eager = opt.flat_p.clone(), eager.losses()
    assert opt.step_count == 2 and len(l_eager) == 2 + tl * (tl - 1) // 2
    graphed = GraphedStep(w, net, opt, batch, use_graph=True, warmup=1, strict=True)
    graphed.run()
    torch.cuda.synchronize()
    assert graphed.mode == 'graph'
    for t, c in zip(state, snap):
        t.copy_(c)
    for _ in range(2):
        graphed.run()
    torch.cuda.synchronize()
    assert opt.step_count == 2
    assert float((opt.flat_p - p_eager).abs().max()) < 2.5e-4
    assert float((opt.flat_p - p_eager).abs().mean()) < 2e-6
    np.testing.assert_allclose(graphed.losses(), l_eager, rtol=2e-3, atol=1e-5)


@pytest.mark.parametrize('tl', [1, 5])
def test_fusenet_rejects_other_track_lengths(tl):
    from depthinspace_amd import synth
    from depthinspace_amd.model import multi_frame_networks
    settings = synth.make_settings(64, 64)
    with pytest.raises(ValueError, match=r'\(2, 3, 4\)'):
        multi_frame_networks.FuseNet((64, 64), settings.K, settings.baseline, track_length=tl)
