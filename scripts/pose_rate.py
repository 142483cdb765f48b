"""Rate of ops.track_poses (csrc/pose.hip) on the MI355X: tracks/s at 512 x 432, tl = 4, iters = 6, with 1 and 4 tracks per call
(profiles/pose_rate.md), the bytes its accumulate passes must read, the share of the HBM figure of BASELINE.md section 4 that comes to,
and - for orientation - the time of the numpy restatement tests/pose_ref.py in float32 on the same input.

Per batch size: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  A caller's workspace is passed; the outputs are allocated by the wrapper, from torch's cache.  The
same call captured once into a hipGraph and replayed in the same windows gives the time of the 2 (iters + 1) launches without the
wrapper's host work (`graph_ms_median`); the byte model is set against that one.

Byte model of one call (n tracks, tl (tl - 1) ordered pairs each, h w pixels, iters + 1 passes; the target is recomputed in every pass,
there is no per-pixel workspace): every pass of every pair reads its frame's disparity (4 B per pixel) and its flow (8 B per pixel);
the four gathered disparities of the other frame are expected to hit in the caches.  The partial sums (256 B per workgroup and pass)
and the state are counted too; they are small.

The joint leg (a second result line per batch size, `leg: joint`) times ops.refine_track_poses in the same session, in the same windows, at
the same number of steps, started from the composed result of the pairwise call just measured, with its status as pair_use.  A joint
pass does the per-pixel work of a pairwise one, so the byte model is the same; `joint_over_pairwise` is the ratio of the two replay
times.  --no-joint leaves the leg out.

    python scripts/pose_rate.py [--h 512 --w 432 --tl 4 --iters 6] [--batches 1 4] [--warmup 3] [--repeats 9] [--calls 50] [--json PATH]
                                [--no-joint]
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


def byte_model(n, tl, h, w, iters, workspace_bytes):
    pairs, passes = n * tl * (tl - 1), iters + 1
    return {'disparity': pairs * passes * h * w * 4, 'flow': pairs * passes * h * w * 8,
            'partial_sums_and_state': 2 * passes * workspace_bytes}      # written by one launch, read by the next: an upper bound


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--iters', type=int, default=6)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4], help='tracks per call')
    ap.add_argument('--no-joint', action='store_true', help='leave out the leg of ops.refine_track_poses')
    add_timing_args(ap)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from tests import pose_inputs, pose_ref
    if not torch.cuda.is_available():
        raise SystemExit('pose_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    lines = []
    for n in a.batches:
        batch = synth.make_batch(st, n, tl=a.tl, seed=7, scene='bumps', motion=0.1, with_primary=False)
        disp_h = np.ascontiguousarray(batch['disp0'][:, :, 0])
        flow_h = pose_inputs.stack_flows(lambda i, j: batch[f'flow_{i}{j}'][:, 0], n, a.tl, a.h, a.w)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        disp, flow = up(disp_h), up(flow_h)
        ws = torch.empty(lib.fn('dis_pose_workspace')(n, a.tl, a.h, a.w), dtype=torch.uint8, device='cuda')
        call = lambda: ops.track_poses(disp, flow, st.K, st.baseline, iters=a.iters, workspace=ws)
        ms, gms, r, rg = time_call(call, a.warmup, a.repeats, a.calls)
        gmed = statistics.median(gms)
        same = all(bool(torch.equal(rg[k].view(torch.int32), r[k].view(torch.int32))) for k in r)
        model = byte_model(n, a.tl, a.h, a.w, a.iters, int(ws.numel()))
        total = sum(model.values())
        truth = pose_inputs.pair_truth(batch['R'], batch['t'])
        res = {'h': a.h, 'w': a.w, 'n': n, 'tl': a.tl, 'iters': a.iters, 'launches': 2 * (a.iters + 1),
               **timing_fields(n, ms, gms), 'graph_equals_eager': same,
               'us_per_launch': round(gmed * 1e3 / (2 * (a.iters + 1)), 2), 'pairs': n * a.tl * (a.tl - 1),
               'pairs_ok': int((r['stats'][..., 3] == 1).sum().item()) - n * a.tl,
               'max_R_error': float(np.abs(r['R_pair'].cpu().numpy() - truth[0]).max()),
               'max_t_error': float(np.abs(r['t_pair'].cpu().numpy() - truth[1]).max()),
               'model_bytes': total, 'model_bytes_by_array': model, 'achieved_GB_per_s': round(total / gmed / 1e6, 1),
               'share_of_hbm': round(total / (gmed * 1e-3) / HBM_BYTES_PER_S, 4), 'model_ms_at_hbm': round(total / HBM_BYTES_PER_S * 1e3, 4),
               'workspace_bytes': int(ws.numel())}
        if n == a.batches[0]:
            t0 = time.perf_counter()
            ref = pose_ref.track_poses(disp_h, flow_h, st.K, st.baseline, iters=a.iters, dtype=np.float32)
            res['numpy_float32_s'] = round(time.perf_counter() - t0, 3)
            res['n_used_equal_to_numpy'] = bool(np.array_equal(ref['stats'][..., 0], r['stats'][..., 0].cpu().numpy()))
            res['max_R_distance_to_numpy'] = float(np.abs(ref['R_pair'] - r['R_pair'].cpu().numpy()).max())
        print(json.dumps(res))
        lines.append(res)
        if a.no_joint:
            continue
        from depthinspace_amd.data.presave_pose import compose_track
        Rp, tp, stat = (r[k].cpu().numpy() for k in ('R_pair', 't_pair', 'stats'))
        starts = [compose_track(Rp[b], tp[b], stat[b, ..., 3] != 0) for b in range(n)]
        R0, t0 = up(np.stack([s_[0] for s_ in starts])), up(np.stack([s_[1] for s_ in starts]))
        use = (r['stats'][..., 3] != 0).to(torch.uint8).contiguous()
        wsj = torch.empty(lib.fn('dis_pose_joint_workspace')(n, a.tl, a.h, a.w), dtype=torch.uint8, device='cuda')
        jcall = lambda: ops.refine_track_poses(disp, flow, st.K, st.baseline, R0, t0, use, iters=a.iters, workspace=wsj)
        jms, jgms, j, jg = time_call(jcall, a.warmup, a.repeats, a.calls)
        jmed = statistics.median(jgms)
        jR, jt = pose_inputs.pair_truth(j['R'].cpu().numpy(), j['t'].cpu().numpy())
        world = pose_inputs.pair_truth(batch['R'], batch['t'])
        jres = {'leg': 'joint', 'h': a.h, 'w': a.w, 'n': n, 'tl': a.tl, 'iters': a.iters, 'launches': 2 * (a.iters + 1),
                **timing_fields(n, jms, jgms), 'graph_equals_eager': all(bool(torch.equal(jg[k].view(torch.int32), j[k].view(torch.int32))) for k in j),
                'us_per_launch': round(jmed * 1e3 / (2 * (a.iters + 1)), 2), 'joint_over_pairwise': round(jmed / gmed, 4),
                'tracks_ok': int((j['track_stats'][:, 3] == 1).sum().item()),
                'contributing_pairs': int(j['track_stats'][:, 0].sum().item()),
                'max_R_error': float(np.abs(jR - world[0]).max()), 'max_t_error': float(np.abs(jt - world[1]).max()),
                'model_bytes': total, 'achieved_GB_per_s': round(total / jmed / 1e6, 1), 'workspace_bytes': int(wsj.numel())}
        print(json.dumps(jres))
        lines.append(jres)
    emit(lines, a.json)


if __name__ == '__main__':
    main()
