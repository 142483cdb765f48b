"""Per-form time of the strict-split fused 3x3 conv backward (dis_conv2d_bwd_fused_bf16x3) against the two launches it replaces, at
the layer shapes of one DIS-MF training step (bench.py's workload: bs = 4, 512 x 432).

One eager step under the three-term split records the form (plain / plain_accum / act / act_accum / xgn) and shape of every fused call
the dispatch makes.  Each distinct (form, shape) is then timed on random operands as the fused call and as the unfused pair (input
gradient + weight gradient, each with its slab reduce), in alternating rounds, median per round of REPS back-to-back calls.  Prints one
JSON line per form: calls per step, fused and two-launch milliseconds per step, their ratio.

    python scripts/bwd_fused_strict_forms.py [--reps 10 --rounds 7]      (on an MI355X)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

C = 32


def step_calls():
    """form and shape of every dis_conv2d_bwd_fused_bf16x3 call of one eager strict DIS-MF step"""
    import bench
    from depthinspace_amd import lib, synth
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    settings = synth.make_settings(bench.H, bench.W)
    torch.manual_seed(0)
    net = multi_frame_networks.FuseNet(imsize=(bench.H, bench.W), K=settings.K, baseline=settings.baseline, track_length=bench.TL,
                                       max_disp=128).cuda()
    wk = multi_frame_worker.Worker(bench.make_args(4), settings=settings)
    wk.build_losses()
    wk.current_epoch = 2
    opt = FlatAdam(net.parameters(), lr=1e-4)
    batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(settings, 4, bench.TL, seed=1234).items()}
    seen = []
    call = lib.call

    def rec(name, *args, _soft=False):
        if name == 'dis_conv2d_bwd_fused_bf16x3':
            in_act, acc, st, gb, n, h, w = args[2], args[8], args[10], args[15], args[17], args[18], args[19]
            form = 'xgn' if st is not None else ('act' if in_act else 'plain') + ('_accum' if acc else '')
            seen.append((form, n, h, w, gb is not None))
        return call(name, *args, _soft=_soft)
    lib.call = rec
    try:
        wk.train_step(net, opt, batch)
        torch.cuda.synchronize()
    finally:
        lib.call = call
    return seen


def pair(form, n, h, w, bias):
    """-> (fused(), unfused()) closures over preallocated random operands of one layer"""
    from depthinspace_amd import lib, ops
    g = torch.Generator().manual_seed(n * 100003 + h * 1009 + w)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    gq, q, x, gx = rnd(n, h, w, C), F.selu(rnd(n, h, w, C)), rnd(n, h, w, C), rnd(n, h, w, C)
    wt = (rnd(C, C, 3, 3) * 0.05).contiguous()
    act, acc = form.startswith('act'), 1 if form.endswith('accum') else 0
    st = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
    gam, bet = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    gw = torch.empty(C, C, 3, 3, device='cuda')
    gb = torch.empty(C, device='cuda') if bias else None
    ws3 = torch.empty(lib.fn('dis_conv2d_bwd_fused_bf16x3_workspace')(C), dtype=torch.float32, device='cuda')
    ws = torch.empty(lib.fn('dis_conv2d_wgrad_workspace')(C, C, 3, 1), dtype=torch.float32, device='cuda')
    xg = (st, gam, bet, 1e-5) if form == 'xgn' else (None, None, None, 0.0)

    def fused():
        lib.call('dis_conv2d_bwd_fused_bf16x3', gq, q if act else None, ops.ACT_SELU if act else 0, wt, C, C, wt.stride(0), gx, acc, x,
                 *xg, gw, gb, ws3, n, h, w, C, 0)

    def unfused():
        if act:
            lib.call('dis_conv2d_dgrad_bf16x3_act', gq, q, ops.ACT_SELU, wt, C, C, wt.stride(0), gx, n, h, w, C, C, 1, acc)
            lib.call('dis_conv2d_wgrad_bf16x3_act', x, gq, q, ops.ACT_SELU, gw, gb, ws, n, h, w, C, C, C, 3, 1, 1)
            return
        lib.call('dis_conv2d_fwd_bf16x3_oihw', gq, wt, 1, C, C, wt.stride(0), None, gx, None, n, h, w, C, C, 3, 1, 1,
                 ops.CONV_ACCUM if acc else 0)
        if form == 'xgn':
            lib.call('dis_conv2d_wgrad_bf16x3_gn', x, *xg, gq, gw, gb, ws, n, h, w, C, C, C, 3, 1, 1)
        else:
            lib.call('dis_conv2d_wgrad_bf16x3', x, gq, gw, gb, ws, n, h, w, C, C, C, 3, 1, 1)
    return fused, unfused


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    from depthinspace_amd import lib
    assert lib.fn('dis_set_conv_split')(0) == 0   # the three-term split
    calls = step_calls()
    per_form = {}
    for key in sorted(set(calls)):
        fused, unfused = pair(*key)
        for f in (fused, unfused, fused, unfused):   # (warm-up: first-launch attributes, caches)
            f()
        tf, tu = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused, args.reps))
            tu.append(timed(unfused, args.reps))
        k = calls.count(key)
        mf, mu = sorted(tf)[len(tf) // 2], sorted(tu)[len(tu) // 2]
        print(json.dumps({'form': key[0], 'n_h_w': key[1:4], 'bias': key[4], 'calls_per_step': k, 'fused_ms': round(mf, 4),
                          'two_launch_ms': round(mu, 4)}))
        d = per_form.setdefault(key[0], [0, 0.0, 0.0])
        d[0] += k
        d[1] += k * mf
        d[2] += k * mu
    for form, (k, mf, mu) in sorted(per_form.items()):
        print(json.dumps({'form': form, 'calls_per_step': k, 'fused_ms_per_step': round(mf, 3), 'two_launch_ms_per_step': round(mu, 3),
                          'fused_over_two_launch': round(mf / mu, 3)}))


if __name__ == '__main__':
    main()
