"""Rate of ops.fuse_track (csrc/fuse.hip) on the MI355X: tracks/s at 512 x 432, tl = 4, with 1 and 4 tracks per call
(profiles/fuse_rate.md), the bytes its three launches must move, the share of the HBM figure of BASELINE.md section 4 that comes to,
and - for orientation - the time of the numpy restatement tests/fuse_ref.py in float32 on the same input.

Per batch size: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  A caller's workspace is passed; the outputs are allocated by the wrapper, from torch's cache.  The
same call captured once into a hipGraph and replayed in the same windows gives the time of the three launches without the wrapper's
host work (`graph_ms_median`); the byte model is set against that one.

Byte model of one call (P = n tl h w pixels, m kept records; what has to move if every array crossed the memory once per launch that
uses it - the 4 neighbours of the normal and the 4 (tl - 1) gathered taps are expected to hit in the caches):
    check     reads  P 4 (disp)                      writes P (1 + 1 + 1 + 4 + 12 + 12) (views, seen, keep, resid, point, normal)
    scan      reads  P / 256 x 4                     writes P / 256 x 4
    scatter   reads  P 1 (keep) + m (12 + 12 + 4)    writes m (12 + 12 + 4 + 4)

    python scripts/fuse_rate.py [--h 512 --w 432 --tl 4] [--batches 1 4] [--warmup 3] [--repeats 9] [--calls 50] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import HBM_BYTES_PER_S, add_timing_args, emit, time_call, timing_fields   # noqa: E402


def byte_model(pixels, kept):
    blocks = -(-pixels // 256)
    return {'check': pixels * 4 + pixels * 31, 'scan': blocks * 8, 'scatter': pixels + kept * 28 + kept * 32}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4], help='tracks per call')
    ap.add_argument('--tol', type=float, default=0.01)
    ap.add_argument('--min-views', type=int, default=2)
    add_timing_args(ap)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from tests import fuse_ref
    if not torch.cuda.is_available():
        raise SystemExit('fuse_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    lines = []
    for n in a.batches:
        batch = synth.make_batch(st, n, tl=a.tl, seed=7, scene='bumps', motion=0.1, with_primary=False, with_flow=False)
        disp_h = np.ascontiguousarray(batch['disp0'][:, :, 0])
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        disp, R, t, val = up(disp_h), up(batch['R']), up(batch['t']), up(batch['ambient0'][:, :, 0])
        ws = torch.empty(lib.fn('dis_fuse_workspace')(n, a.tl, a.h, a.w), dtype=torch.uint8, device='cuda')
        call = lambda: ops.fuse_track(disp, R, t, st.K, st.baseline, val, tol=a.tol, min_views=a.min_views, workspace=ws)
        ms, gms, r, rg = time_call(call, a.warmup, a.repeats, a.calls)
        gmed = statistics.median(gms)
        kept = int(r['count'].sum().item())
        same = all(bool(torch.equal(rg[k][:kept] if k != 'count' else rg[k], r[k][:kept] if k != 'count' else r[k])) for k in r)
        pixels = n * a.tl * a.h * a.w
        model = byte_model(pixels, kept)
        total = sum(model.values())
        res = {'h': a.h, 'w': a.w, 'n': n, 'tl': a.tl, 'tol': a.tol, 'min_views': a.min_views, 'launches': 3,
               **timing_fields(n, ms, gms), 'graph_equals_eager': same,
               'pixels': pixels, 'kept': kept, 'model_bytes': total, 'model_bytes_by_launch': model,
               'achieved_GB_per_s': round(total / gmed / 1e6, 1), 'share_of_hbm': round(total / (gmed * 1e-3) / HBM_BYTES_PER_S, 4),
               'model_ms_at_hbm': round(total / HBM_BYTES_PER_S * 1e3, 4), 'workspace_bytes': int(ws.numel())}
        if n == a.batches[0]:
            t0 = time.perf_counter()
            ref = fuse_ref.fuse(disp_h, batch['R'], batch['t'], st.K, st.baseline, batch['ambient0'][:, :, 0], a.tol, a.min_views,
                                dtype=np.float32)
            res['numpy_float32_s'] = round(time.perf_counter() - t0, 3)
            res['numpy_kept'] = int(ref['count'].sum())
            res['src_equal_to_numpy'] = bool(np.array_equal(ref['src'], r['src'][:kept].cpu().numpy()))
        print(json.dumps(res))
        lines.append(res)
    emit(lines, a.json)


if __name__ == '__main__':
    main()
