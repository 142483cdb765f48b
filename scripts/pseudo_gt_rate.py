"""Time of the masked pseudo-GT term, ops.masked_l1_multi (csrc/pixel_ops.hip), on the MI355X: forward + backward of n = 4 estimates
against one target of `--planes` x 512 x 432 with about 30 % holes, at erode 0 and 1, next to the four ops.l1_mean forward +
backward calls on a hole-free target that the default pseudo-GT path makes (profiles/pseudo_gt_rate.md).

A call here is the value(s) and the gradients of all four estimates: the entry points the two ops.py nodes call, in their order, on
buffers allocated once (forward, then backward with unit incoming gradients) - 3 launches for the masked form, 12 and the zero-fill of
the four accumulators for the other; autograd's own host work is in neither.  Each figure: `--warmup` untimed calls, then `--repeats`
windows of `--calls` calls each, every window between two HIP events; the median window gives the call time.  The same call captured
once into a hipGraph and replayed in the same windows gives the time without the wrappers' host work.  The three forms are timed in
turn, `--rounds` times over, so that a drift of the machine shows as a spread between rounds and not as a difference between forms.

    python scripts/pseudo_gt_rate.py [--h 512 --w 432 --planes 32] [--holes 0.3] [--rounds 3] [--warmup 3] [--repeats 9] [--calls 50] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rate_common as RC   # noqa: E402


def holed_target(rng, planes, h, w, share):
    """a positive target with rectangular holes (0) over about `share` of its pixels -> (float32 (planes, 1, h, w), the share)"""
    import numpy as np
    t = (rng.rand(planes, 1, h, w) * 60 + 0.5).astype(np.float32)
    hole = np.zeros((planes, 1, h, w), dtype=bool)
    while hole.mean() < share:
        p, y, x = rng.randint(planes), rng.randint(h), rng.randint(w)
        hole[p, 0, y:y + rng.randint(8, h // 3), x:x + rng.randint(8, w // 3)] = True
    t[hole] = 0
    return t, float(hole.mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--planes', type=int, default=32, help='tl * bs')
    ap.add_argument('--holes', type=float, default=0.3)
    ap.add_argument('--rounds', type=int, default=3)
    RC.add_timing_args(ap, calls=50)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops
    if not torch.cuda.is_available():
        raise SystemExit('pseudo_gt_rate.py measures on the GPU: no device found')
    rng = np.random.RandomState(5)
    t_np, share = holed_target(rng, a.planes, a.h, a.w, a.holes)
    full_np = np.where(t_np > 0, t_np, np.float32(1.0)).astype(np.float32)
    holed, full = torch.from_numpy(t_np).cuda(), torch.from_numpy(full_np).cuda()
    outs = [torch.from_numpy((full_np + rng.randn(*full_np.shape) * (k + 1)).astype(np.float32)).cuda() for k in range(4)]
    # everything a call writes is allocated here: a call is its launches and nothing else, eagerly and captured
    grads = [torch.empty_like(o) for o in outs]
    ones, vals = torch.ones(4, device='cuda'), torch.empty(4, device='cuda')
    acc = torch.empty(lib.fn('dis_masked_l1_multi_acc_doubles')(), dtype=torch.float64, device='cuda')
    acc1 = torch.zeros(4, dtype=torch.float64, device='cuda')
    est, gtab = ops._ptr_table(outs), ops._ptr_table(grads)
    count = full.numel()

    def masked(r):
        def call():
            lib.call('dis_masked_l1_multi_fwd', est, 4, holed, r, acc, vals, a.planes, a.h, a.w)
            lib.call('dis_masked_l1_multi_bwd', est, 4, holed, r, acc, ones, gtab, a.planes, a.h, a.w)
            return vals
        return call

    def four_l1():
        acc1.zero_()                          # (ops.l1_mean hands every call a zeroed double)
        for k in range(4):
            lib.call('dis_l1_mean_fwd', outs[k], full, acc1[k:k + 1], vals[k:k + 1], count)
        for k in range(4):
            lib.call('dis_l1_mean_bwd', outs[k], full, ones[k:k + 1], grads[k], count)
        return vals

    forms = (('masked_erode0', masked(0)), ('masked_erode1', masked(1)), ('four_l1_mean', four_l1))
    arr = a.planes * a.h * a.w * 4
    res = {'h': a.h, 'w': a.w, 'planes': a.planes, 'n': 4, 'hole_share': round(share, 4), 'array_bytes': arr,
           # what the algorithm has to move per forward + backward: each estimate read twice and its gradient written, the target read
           # once per launch by the masked form (two launches that touch it) and once per l1_mean launch (eight) by the other
           'bytes_masked': (4 * 3 + 2) * arr, 'bytes_four_l1_mean': (4 * 3 + 8) * arr, 'rounds': []}
    for _ in range(a.rounds):
        rd = {}
        for name, fn in forms:
            ms, gms, _, _ = RC.time_call(fn, a.warmup, a.repeats, a.calls)
            rd[name] = {**RC.ms_fields('call_ms', ms), **RC.ms_fields('graph_ms', gms)}
        res['rounds'].append(rd)
    print(json.dumps(res))
    RC.emit(res, a.json)


if __name__ == '__main__':
    main()
