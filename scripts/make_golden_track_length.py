"""Step fixtures at track lengths 2 and 3: tests/golden/{mf,sf}_*_tl{2,3}_*.npz, from the reference itself on CPU.

oracle/make_golden.py writes the tl = 4 fixtures; this script runs the same recipe with the reference's
`FuseNet(track_length=tl)` / `DispDecoder` and a worker whose `track_length` is tl, on `synth.make_batch(settings, bs, tl)`
(or `make_random_batch`).  It reuses oracle/make_golden.py's import shims and reference worker, and writes the same key
schema as the tl = 4 step fixtures plus `tl`.  The CPU oracle (`StepContext(tl=tl)`, `mf_param_shapes(tl=tl)`) is run on
the same inputs and must agree with the reference, as in make_golden.run_step_case.

    python scripts/make_golden_track_length.py                 # all cases into tests/golden
    python scripts/make_golden_track_length.py --out DIR NAME  # selected cases elsewhere

Needs the reference checkout (the build container only)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402

CASES = [
    ('mf_64_tl2_bs1', dict(arch='multi_frame', tl=2, size=(64, 64), bs=1, pseed=31, bseed=1234, epoch=0)),
    ('mf_64_tl3_bs2_rnd', dict(arch='multi_frame', tl=3, size=(64, 64), bs=2, pseed=32, bseed=99, epoch=2, random_batch=True)),
    ('mf_128_tl3_bs1', dict(arch='multi_frame', tl=3, size=(128, 128), bs=1, pseed=33, bseed=1234, epoch=2)),
    # DIS-SF only meets tl in its losses: a cheap confirmation that it already follows it
    ('sf_64_tl2_bs1', dict(arch='single_frame', tl=2, size=(64, 64), bs=1, pseed=34, bseed=1234)),
]


def run_case(ref, arch, tl, size, bs, pseed, bseed, epoch=0, random_batch=False):
    from depthinspace_amd import synth
    from oracle import dis_oracle as O
    H, W = size
    settings = synth.make_settings(H, W)
    mk = synth.make_random_batch if random_batch else synth.make_batch
    batch = mk(settings, bs, tl, seed=bseed)
    mf = arch == 'multi_frame'
    shapes = O.mf_param_shapes(tl=tl) if mf else O.sf_param_shapes()
    params = O.init_params(shapes, seed=pseed)

    # ---- reference
    if mf:
        net = ref['mfn'].FuseNet(imsize=(H, W), K=settings.K, baseline=settings.baseline, track_length=tl, max_disp=128)
    else:
        imsizes = [(H, W)]
        for _ in range(3):
            imsizes.append((imsizes[-1][0] // 2, imsizes[-1][1] // 2))
        net = ref['networks'].DispDecoder(channels_in=2, max_disp=128, imsizes=imsizes)
    sd = net.state_dict()
    assert sorted(sd.keys()) == sorted(shapes.keys()), set(sd.keys()) ^ set(shapes.keys())
    for k in sd:
        assert tuple(sd[k].shape) == tuple(shapes[k]), (k, sd[k].shape, shapes[k])
    net.load_state_dict({k: v.detach().clone() for k, v in params.items()})
    net.train()
    w = MG.ref_worker(ref, arch, settings, epoch)
    w.track_length = tl
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    w.copy_data(MG.to_torch_batch(batch), 'cpu', False, True)
    opt.zero_grad()
    flow = w.read_optical_flow(True)
    # the reference's own torch.topk ids (Conv3D, multi_frame_networks.py:498): 8 tl calls per forward = 4 blocks x
    # (conv3d_1, conv3d_2) x tl target frames, each (bs*ho*wo, 9, 1)
    ref_topk = []
    _topk = torch.topk

    def _rec_topk(*a, **k):
        r = _topk(*a, **k)
        ref_topk.append(r[1].detach().clone())
        return r
    torch.topk = _rec_topk
    try:
        out = w.net_forward(net, flow)
    finally:
        torch.topk = _topk
    vals = w.loss_forward(out, True, flow)
    sum(vals).backward()
    ref_grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in net.named_parameters()}
    opt.step()
    ref_new = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ref_data = {k: v.detach().clone() for k, v in w.data.items() if k in ('im0', 'std0')}
    outs = out if isinstance(out, (list, tuple)) else [out]

    # ---- oracle
    ctx = O.StepContext(settings, tl=tl)
    st = {'step': 0, 'm': {}, 'v': {}}
    O.CONV3D_TAP = [] if mf else None
    res = O.train_step(ctx, arch, params, MG.to_torch_batch(batch), adam_state=st, epoch=epoch)
    tap, O.CONV3D_TAP = O.CONV3D_TAP, None
    o_outs = res['out'] if isinstance(res['out'], (list, tuple)) else [res['out']]
    assert len(vals) == len(res['vals'])
    rep = {'out': max(MG.maxdiff(a, b) for a, b in zip(outs, o_outs)),
           'vals': max(abs(float(a.detach()) - float(b.detach())) for a, b in zip(vals, res['vals'])),
           'im0': MG.maxdiff(ref_data['im0'], res['data']['im0']), 'std0': MG.maxdiff(ref_data['std0'], res['data']['std0'])}
    gd = 0.0
    for k, g in ref_grads.items():
        og = res['grads'][k]
        if g is None:
            assert og is None or float(og.abs().max()) == 0.0, k
            continue
        gd = max(gd, MG.maxdiff(g, og) / (float(g.abs().max()) + 1e-12))
    rep['grad_rel'] = gd
    rep['adam'] = max(MG.maxdiff(ref_new[k], params[k]) for k in params)
    print(f'[{arch} tl={tl} {H}x{W} bs={bs} epoch={epoch} rnd={random_batch}] oracle-vs-reference:', rep)
    # the oracle restates the reference (tests/test_oracle_golden.py's bars; Adam's first step is lr = 1e-4 times the sign of the
    # gradient where that is well above eps, so gradients near 0 may move a parameter by a fraction of a step)
    assert rep['out'] < 1e-5 and rep['vals'] < 1e-6 and rep['grad_rel'] < 2e-5 and rep['adam'] < 2e-5, rep

    fx = {'arch': arch, 'tl': tl, 'H': H, 'W': W, 'bs': bs, 'pseed': pseed, 'bseed': bseed, 'epoch': epoch,
          'use_pseudo_gt': 0, 'random_batch': int(random_batch), 'pattern': 'default', 'scene': 'plane', 'motion': 1.0,
          'torch_threads': torch.get_num_threads(), 'vals': np.array([float(v) for v in vals], dtype=np.float64)}
    for i, o in enumerate(outs):
        fx[f'out{i}'] = o.detach().numpy()
    fx['std0_sum'] = np.float64(ref_data['std0'].double().sum())
    fx['im0_lcn_sample'] = ref_data['im0'][:, :, 0, ::7, ::5].numpy()
    if mf:
        assert len(ref_topk) == 8 * tl, len(ref_topk)
        for li, (lname, tag) in enumerate((('conv3d_1', 'core'), ('conv3d_2', 'quarter'))):
            per_block = []
            for b in range(4):
                calls = [c for c in tap if c['name'] == f'blocks.{b}.{lname}']
                assert [c['target'] for c in calls] == list(range(tl))
                per_block.append(torch.stack([c['idx'] for c in calls], 0))  # (tl,bs,ho,wo,9)
            for b in range(1, 4):
                assert bool((torch.sort(per_block[b], -1)[0] == torch.sort(per_block[0], -1)[0]).all())
            # the reference module's own torch.topk output (block-major, layer, target), element for element and in order
            ids = torch.stack([ref_topk[li * tl + ti].view(per_block[0][ti].shape) for ti in range(tl)], 0)
            for b in range(4):
                for ti in range(tl):
                    r = ref_topk[b * 2 * tl + li * tl + ti]
                    assert bool((r.view(ids[ti].shape) == ids[ti]).all()), (lname, b, ti)
            assert bool((ids == per_block[0]).all()), lname   # ... which the oracle reproduces
            fx[f'knn_idx_{tag}'] = ids.numpy().astype(np.uint8)
            keysrt = torch.sort(torch.stack([c['key'] for c in tap if c['name'] == f'blocks.0.{lname}'], 0), -1)[0]
            k9, k10 = keysrt[..., 8].double(), keysrt[..., 9].double()
            fx[f'knn_margin_{tag}'] = ((k10 - k9) / torch.clamp(k10, min=1e-30)).float().numpy()
    keys = sorted(ref_grads.keys())
    fx['grad_keys'] = np.array(keys)
    fx['grad_absmax'] = np.array([0.0 if ref_grads[k] is None else float(ref_grads[k].abs().max()) for k in keys])
    fx['grad_sum'] = np.array([0.0 if ref_grads[k] is None else float(ref_grads[k].double().sum()) for k in keys])
    fx['grad_l2'] = np.array([0.0 if ref_grads[k] is None else float(ref_grads[k].double().norm()) for k in keys])
    fx['grad_none'] = np.array([ref_grads[k] is None for k in keys])
    for k in keys:
        g = ref_grads[k]
        if g is not None and g.numel() <= 4096:
            fx['grad:' + k] = g.numpy()
            fx['new:' + k] = ref_new[k].numpy()
    return fx


def main():
    args = sys.argv[1:]
    out_dir = MG.GOLD
    if '--out' in args:
        i = args.index('--out')
        out_dir = args[i + 1]
        args = args[:i] + args[i + 2:]
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = MG.import_reference()
    for name, kw in CASES:
        if args and name not in args:
            continue
        fx = run_case(ref, **kw)
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **fx)
        print(name, 'written', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
