"""Rate of ops.disp_align_poses (csrc/disp_align.hip) on the MI355X: tracks/s at 512 x 432, tl = 4, with 1 and 4 tracks per call
(profiles/disp_align_rate.md), for the default schedule and for cheaper ones, with the pose error each schedule leaves on rendered
tracks (data/render.py: render_batch, exact disparities, and the same with Gaussian noise of --noise px), and the rate of ops.rigid_flow.

Per batch size and schedule: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP
events; the median window gives the call time.  A caller's workspace is passed; the outputs are allocated by the wrapper, from torch's
cache.  The same call captured once into a hipGraph and replayed in the same windows gives the time of the launches without the
wrapper's host work (`graph_ms_median`).  The split between the pyramid, the accumulate and the solve launches comes from a separate
run under a kernel trace (the kernels are dalign_down_kernel, dalign_maps_kernel, dalign_accum_kernel, dalign_solve_kernel).

Byte model of one call (n tracks, tl frames, tl (tl - 1) ordered pairs each): a pass at level l reads, per pair, frame i's disparities
(4 B per pixel of the level) and - each map pixel once, the four taps of neighbouring pixels sharing lines - frame j's maps (16 B per
pixel); the pyramid and the maps are written and read once per frame and level (4 + 16 B per pixel written, 4 B read).

    python scripts/disp_align_rate.py [--h 512 --w 432 --tl 4] [--batches 1 4] [--schedules 10,6,4,4,4 4,4,4,4,4] [--noise 0.05]
                                      [--warmup 3] [--repeats 9] [--calls 20] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import HBM_BYTES_PER_S, add_timing_args, emit, time_call, timing_fields   # noqa: E402


def byte_model(n, tl, sizes, iters):
    frames, pairs = n * tl, n * tl * (tl - 1)
    px = [a * b for a, b in sizes]
    passes = [int(v) for v in iters]
    passes[0] += 1                                                   # the closing pass
    return {'pyramid_and_maps': frames * sum(p * (4 + 4 + 16) for p in px),
            'accumulate': pairs * sum(k * p * (4 + 16) for k, p in zip(passes, px))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4], help='tracks per call')
    ap.add_argument('--schedules', nargs='+', default=None, help='steps per level, finest first, comma separated; default: the default one and 4 everywhere')
    ap.add_argument('--noise', type=float, default=0.05, help='sigma of the disparity noise of the second accuracy leg, px')
    ap.add_argument('--seed', type=int, default=3)
    add_timing_args(ap, calls=20)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from depthinspace_amd.data import presave_pose as PP, render
    if not torch.cuda.is_available():
        raise SystemExit('disp_align_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    levels = ops.disp_align_levels(a.h, a.w)
    sizes = ops.disp_align_level_sizes(a.h, a.w, levels)
    schedules = ([tuple(ops.DISP_ALIGN_ITERS[:levels]), (4,) * levels] if a.schedules is None
                 else [tuple(int(v) for v in s.split(',')) for s in a.schedules])
    lines = []
    for n in a.batches:
        batch = render.render_batch(st, n, a.tl, seed=a.seed)
        disp = batch['disp0'][:, :, 0].contiguous()
        noisy = torch.where(disp > 0, disp + a.noise * torch.randn(disp.shape, generator=torch.Generator('cuda').manual_seed(5), device='cuda'), disp)
        Rt, tt = (torch.as_tensor(batch[k]).cpu().numpy() for k in ("R", "t"))
        truth = [PP.relative_poses(Rt[b], tt[b]) for b in range(n)]
        off = ~np.eye(a.tl, dtype=bool)
        depth = [PP.median_depth(disp[b].cpu().numpy(), float(st.K[0, 0]) * float(st.baseline)) for b in range(n)]
        motion = np.concatenate([PP.rotation_angle(truth[b][0])[off] for b in range(n)])
        ws = torch.empty(lib.fn('dis_disp_align_workspace')(n, a.tl, a.h, a.w, levels), dtype=torch.uint8, device='cuda')

        def errors(r):
            Rp, tp, s = (r[k].cpu().numpy() for k in ('R_pair', 't_pair', 'stats'))
            rot = np.concatenate([PP.rotation_angle(Rp[b] @ np.swapaxes(truth[b][0], -1, -2))[off] for b in range(n)])
            tr = np.concatenate([(np.linalg.norm(tp[b] - truth[b][1], axis=-1) / depth[b])[off] for b in range(n)])
            return {'rot_mean': float(rot.mean()), 'rot_max': float(rot.max()), 'trans_mean': float(tr.mean()), 'trans_max': float(tr.max()),
                    'pairs_ok': int((s[..., 3] == 1).sum()) - n * a.tl, 'share_used': float((s[..., 0] / (a.h * a.w))[:, off].mean()),
                    'rms_residual': float(s[..., 2][:, off].mean())}

        for it in schedules:
            call = lambda: ops.disp_align_poses(disp, st.K, st.baseline, levels=levels, iters=it, workspace=ws)
            ms, gms, r, rg = time_call(call, a.warmup, a.repeats, a.calls)
            gmed = statistics.median(gms)
            model = byte_model(n, a.tl, sizes, it)
            total = sum(model.values())
            launches = 2 * levels - 1 + 2 * (sum(it) + 1)
            res = {'h': a.h, 'w': a.w, 'n': n, 'tl': a.tl, 'levels': levels, 'iters': list(it), 'launches': launches,
                   **timing_fields(n, ms, gms), 'graph_equals_eager': all(bool(torch.equal(rg[k].view(torch.int32), r[k].view(torch.int32))) for k in r),
                   'us_per_launch': round(gmed * 1e3 / launches, 2), 'pairs': n * a.tl * (a.tl - 1),
                   'true_rotation_mean': float(motion.mean()), 'true_rotation_max': float(motion.max()),
                   'exact': errors(r), f'noise_{a.noise:g}': errors(ops.disp_align_poses(noisy, st.K, st.baseline, levels=levels, iters=it, workspace=ws)),
                   'model_bytes': total, 'model_bytes_by_part': model, 'achieved_GB_per_s': round(total / gmed / 1e6, 1),
                   'share_of_hbm': round(total / (gmed * 1e-3) / HBM_BYTES_PER_S, 4), 'workspace_bytes': int(ws.numel())}
            print(json.dumps(res))
            lines.append(res)
        # the rigid flow under the poses just estimated (the pairs out of frame 0 as frame poses)
        R0, t0 = r['R_pair'][:, 0].contiguous(), r['t_pair'][:, 0].contiguous()
        fcall = lambda: ops.rigid_flow(disp, R0, t0, st.K, st.baseline, want_visible=True)
        fms, fgms, fr, _ = time_call(fcall, a.warmup, a.repeats, a.calls)
        fbytes = n * a.tl * a.tl * a.h * a.w * (4 + 8 + 1)            # a disparity in, a flow and a flag out, per pixel and pair
        fres = {'leg': 'rigid_flow', 'h': a.h, 'w': a.w, 'n': n, 'tl': a.tl, **timing_fields(n, fms, fgms), 'model_bytes': fbytes,
                'achieved_GB_per_s': round(fbytes / statistics.median(fgms) / 1e6, 1), 'visible_share': float(fr[1].float().mean().item())}
        print(json.dumps(fres))
        lines.append(fres)
    emit(lines, a.json)


if __name__ == '__main__':
    main()
