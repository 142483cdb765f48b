"""Rate of ops.dense_flow (csrc/flow.hip) on the MI355X: tracks/s and pairs/s at 512 x 432, tl = 4, the default parameters
(profiles/flow_rate.md), with the Jacobi steps run 8 per launch on an LDS-resident tile (variant 0, what ships) and one per launch
from memory (variant 1) in the same process.

Per variant: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  Both variants give the same bits (checked here on the timed input).  The launch count and the
byte model below are whole-call figures.

Byte model of one call (P = n tl (tl - 1) pairs; per level of h x w pixels, `warps` linearisations of `iters` steps; what has to move if
every array crossed the memory once per launch that uses it):
    warp        reads  P h w (2 flow + 1 a + 4 b taps) 4        writes P h w 3 x 4
    solve       variant 0, per launch of up to 8 steps: reads P h w (2 + 2 + 3) 4 x (64 x 48) / (48 x 32) (the halo), writes P h w 2 x 4
                variant 1, per step:                    reads P h w (2 + 2 + 3) 4 (the 8 neighbours are expected to hit in the caches),
                                                        writes P h w 2 x 4
(the pyramid, the upsampling and the final store are a few per cent and left out).

    python scripts/flow_rate.py [--h 512 --w 432 --n 1 --tl 4] [--warmup 3] [--repeats 9] [--calls 3] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rate_common as RC   # noqa: E402


def level_sizes(h, w, min_size):
    from depthinspace_amd import ops
    return ops.flow_level_sizes(h, w, min_size)


def launches(h, w, warps, iters, min_size, variant):
    """launches of one call"""
    nl = len(level_sizes(h, w, min_size))
    solve = iters if variant == 1 else -(-iters // 8)
    return 2 + (nl - 1) + nl * (1 + warps * (1 + solve)) + 1


def byte_model(n, tl, h, w, warps, iters, min_size, variant):
    """-> dict launch family -> bytes of one call"""
    P = n * tl * (tl - 1)
    px = sum(a * b for a, b in level_sizes(h, w, min_size)) * P
    if variant == 1:
        solve = iters * (px * 7 * 4 + px * 8)
    else:
        solve = -(-iters // 8) * (px * 7 * 4 * (64 * 48) // (48 * 32) + px * 8)
    return {'warp': warps * (px * 7 * 4 + px * 12), 'solve': warps * solve}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--n', type=int, default=1, help='tracks per call')
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--alpha', type=float, default=1.0)
    ap.add_argument('--warps', type=int, default=3)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--min-size', type=int, default=8)
    RC.add_timing_args(ap, calls=3)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    if not torch.cuda.is_available():
        raise SystemExit('flow_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    batch = synth.make_batch(st, a.n, tl=a.tl, seed=7, scene='bumps', motion=0.1, with_primary=False)
    frames = torch.from_numpy(np.ascontiguousarray(batch['ambient0'][:, :, 0])).cuda()
    kw = dict(alpha=a.alpha, warps=a.warps, iters=a.iters, min_size=a.min_size)
    ws = torch.empty(lib.fn('dis_flow_workspace')(a.n, a.tl, a.h, a.w, a.min_size), dtype=torch.uint8, device='cuda')
    lines, flows = [], []
    for variant in (0, 1):
        ms, flow = RC.eager(lambda: ops.dense_flow(frames, workspace=ws, variant=variant, **kw), a.warmup, a.repeats, a.calls)
        flows.append(flow)
        med = statistics.median(ms)
        model = byte_model(a.n, a.tl, a.h, a.w, a.warps, a.iters, a.min_size, variant)
        total = sum(model.values())
        f = flow.cpu().numpy().astype(np.float64)
        err, true = [], []
        for i in range(a.tl):
            for j in range(a.tl):
                if i != j:
                    t = batch[f'flow_{i}{j}'][:, 0].astype(np.float64)
                    err.append(np.sqrt(((f[:, i * a.tl + j] - t) ** 2).sum(1)).mean())
                    true.append(np.sqrt((t ** 2).sum(1)).mean())
        res = {'h': a.h, 'w': a.w, 'n': a.n, 'tl': a.tl, 'variant': variant, **kw, 'levels': len(level_sizes(a.h, a.w, a.min_size)),
               'launches': launches(a.h, a.w, a.warps, a.iters, a.min_size, variant),
               **RC.ms_fields('call_ms', ms), 'tracks_per_s': round(a.n / med * 1e3, 2), 'pairs_per_s': round(a.n * a.tl * (a.tl - 1) / med * 1e3, 1),
               'model_bytes': total, 'model_bytes_by_family': model, 'achieved_GB_per_s': round(total / med / 1e6, 1),
               'workspace_bytes': int(ws.numel()), 'mean_true_flow_px': round(float(np.mean(true)), 3),
               'mean_end_point_error_px': round(float(np.mean(err)), 4)}
        print(json.dumps(res))
        lines.append(res)
    same = bool(torch.equal(flows[0], flows[1]))
    print(json.dumps({'variants_give_the_same_bits': same, 'speedup_of_variant_0': round(lines[1]['call_ms_median'] / lines[0]['call_ms_median'], 3)}))
    RC.emit(lines + [{'variants_give_the_same_bits': same}], a.json)


if __name__ == '__main__':
    main()
