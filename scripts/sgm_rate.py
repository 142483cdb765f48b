"""Rate of ops.sgm_disparity (csrc/sgm.hip) on the MI355X: frames/s at 512 x 432, n = 4, ndisp = 64 and 128 (profiles/sgm_rate.md).

Per configuration: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  The achieved GB/s is the byte model below over that time: a whole-call rate (ten launches and the
gaps between them), not a kernel's share of the memory bandwidth.

Byte model of one call (n frames of h x w, D candidates; what the algorithm has to move if every array crossed the memory once per
launch that uses it - the re-reads of the pattern's census row and of the diagonal of S are expected to hit in the caches):
    census      reads  (n + 1) h w 4        writes (n + 1) h w 8
    path x 8    reads  n h w 8 (image census) + h w 8 (pattern census) + n h w D 2 (S; not in the first launch)
                writes n h w D 2
    winner      reads  n h w D 2            writes n h w 4

    python scripts/sgm_rate.py [--h 512 --w 432 --n 4] [--ndisp 64 128] [--warmup 5] [--repeats 15] [--calls 10] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rate_common as RC   # noqa: E402


def byte_model(n, h, w, d):
    """-> dict launch family -> bytes of one call"""
    hw = h * w
    vol = n * hw * d * 2
    return {'census': (n + 1) * hw * 12,
            'paths': 8 * (n * hw * 8 + hw * 8) + 7 * vol + 8 * vol,
            'winner': vol + n * hw * 4}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--n', type=int, default=4)
    ap.add_argument('--ndisp', type=int, nargs='+', default=[64, 128])
    RC.add_timing_args(ap, warmup=5, repeats=15, calls=10)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    if not torch.cuda.is_available():
        raise SystemExit('sgm_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    batch = synth.make_batch(st, 1, tl=a.n, seed=7, scene='bumps', with_flow=False, with_primary=False)
    im = torch.from_numpy(batch['im0'][0]).cuda()
    pat = torch.from_numpy(np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)).cuda()
    truth = torch.from_numpy(batch['disp0'][0]).cuda()
    lines = []
    for d in a.ndisp:
        ws = torch.empty(lib.fn('dis_sgm_workspace')(a.n, a.h, a.w, d), dtype=torch.uint8, device='cuda')
        ms, disp = RC.eager(lambda: ops.sgm_disparity(im, pat, ndisp=d, workspace=ws), a.warmup, a.repeats, a.calls)
        med = statistics.median(ms)
        model = byte_model(a.n, a.h, a.w, d)
        total = sum(model.values())
        valid = disp != 0
        res = {'h': a.h, 'w': a.w, 'n': a.n, 'ndisp': d, **RC.ms_fields('call_ms', ms), 'frames_per_s': round(a.n / med * 1e3, 1), 'model_bytes': total,
               'model_bytes_by_family': model, 'achieved_GB_per_s': round(total / med / 1e6, 1),
               'workspace_bytes': int(ws.numel()), 'valid_fraction': round(float(valid.float().mean()), 4),
               'valid_off_by_more_than_1px': round(float(((disp - truth).abs() > 1)[valid].float().mean()), 4)}
        print(json.dumps(res))
        lines.append(res)
    RC.emit(lines, a.json)


if __name__ == '__main__':
    main()
