"""Rate of ops.tsdf_align_poses (csrc/tsdf_align.hip) on the MI355X: calls/s and views/s at 512 x 432, a lattice of `--res` points
along the longest side placed and integrated as data/mesh.py does it, `--iters` Gauss-Newton steps from poses half a voxel off
(profiles/tsdf_align_rate.md) - for one view and for the track's four, and with the leave-one-out integrations of
data/presave_pose.py --model: one frame (the three other frames integrated by ops.tsdf_integrate, then the frame aligned) and one
round (the frames 1 .. tl - 1 in turn).  Two more legs split the call: `floor`, the same call on disparities that are all invalid - the
launches, the disparity loads, the reduction, the records and the solve launches stay, the sampling of the volume goes - and `one_step`,
the call with one step instead of `--iters` (two pairs of launches instead of `--iters` + 1).

Each figure: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  A caller's workspace is passed.  The same call captured once into a hipGraph and replayed in the
same windows gives the time without the wrapper's host work.

    python scripts/tsdf_align_rate.py [--h 512 --w 432 --tl 4] [--res 256] [--iters 6] [--warmup 3] [--repeats 9] [--calls 20] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rate_common as RC   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--trunc', type=float, default=3.0)
    ap.add_argument('--iters', type=int, default=6)
    RC.add_timing_args(ap, calls=20)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from depthinspace_amd.data import mesh as M
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_align_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    batch = synth.make_batch(st, 1, tl=a.tl, seed=7, scene='bumps', motion=0.1, with_primary=False, with_flow=False)
    disp_h, R_h, t_h = (np.ascontiguousarray(x, dtype=np.float32) for x in (batch['disp0'][0, :, 0], batch['R'][0], batch['t'][0]))
    v = M.integrate_track(disp_h, R_h, t_h, None, st, a.res, None, a.trunc)
    nx, ny, nz = v['grid']
    dev = torch.device('cuda')
    disp = torch.from_numpy(disp_h).to(dev)
    # the starts: every pose moved by half a voxel along x and turned about y by the angle that moves a point at the median depth as far
    half = 0.5 * v['voxel']
    depth = float(np.median(float(st.K[0][0]) * st.baseline / disp_h[disp_h > 0]))
    ang = half / depth
    dR = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    R0 = torch.from_numpy(np.stack([dR @ r for r in R_h.astype(np.float64)]).astype(np.float32)).to(dev)
    t0 = torch.from_numpy(np.stack([dR @ t + np.array([half, 0, 0]) for t in t_h.astype(np.float64)]).astype(np.float32)).to(dev)
    ws = torch.empty(lib.fn('dis_tsdf_align_workspace')(a.tl, a.h, a.w), dtype=torch.uint8, device=dev)

    def align(vol, d, R, t, iters=a.iters):
        return ops.tsdf_align_poses(vol[0], vol[1], v['origin'], v['voxel'], v['trunc'], d, v['K'], st.baseline, R, t, iters=iters, workspace=ws)

    full = (v['tsdf'], v['weight'])
    others = [[k for k in range(a.tl) if k != f] for f in range(a.tl)]
    sub = [(disp[o].contiguous(), v['R'][o].contiguous(), v['t'][o].contiguous()) for o in others]

    def loo(f):
        d, R, t = sub[f]
        tsdf, weight, _ = ops.tsdf_integrate(d, R, t, v['K'], st.baseline, None, origin=v['origin'], voxel=v['voxel'], trunc=v['trunc'], grid=v['grid'])
        return align((tsdf, weight), disp[f:f + 1], R0[f:f + 1], t0[f:f + 1])

    def loo_round():
        return [loo(f) for f in range(1, a.tl)][-1]

    r = align(full, disp, R0, t0)
    torch.cuda.synchronize()
    stats = r['stats'].cpu().numpy()
    res = {'h': a.h, 'w': a.w, 'views': a.tl, 'res': a.res, 'grid': [nx, ny, nz], 'lattice_points': nx * ny * nz, 'voxel': v['voxel'],
           'iters': a.iters, 'workspace_bytes': int(ws.numel()), 'status': stats[:, 3].astype(int).tolist(),
           'used_share': [round(float(s[0] / max(s[7], 1)), 4) for s in stats],
           'rms_voxels_before': [round(float(s[6] / v['voxel']), 4) for s in stats], 'rms_voxels_after': [round(float(s[2] / v['voxel']), 4) for s in stats]}
    zeros = torch.zeros_like(disp)
    legs = (('views1', 1, lambda: align(full, disp[:1], R0[:1], t0[:1])), ('views4', a.tl, lambda: align(full, disp, R0, t0)),
            ('views4_floor', a.tl, lambda: align(full, zeros, R0, t0)), ('views4_one_step', a.tl, lambda: align(full, disp, R0, t0, iters=1)),
            ('loo_frame', 1, lambda: loo(1)), ('loo_round', a.tl - 1, loo_round))
    for name, n, fn in legs:
        ms, gms, _, _ = RC.time_call(fn, a.warmup, a.repeats, a.calls)
        f = RC.timing_fields(n, ms, gms)
        f['views_per_s'], f['graph_views_per_s'] = f.pop('tracks_per_s'), f.pop('graph_tracks_per_s')
        res[name] = f
    g = lambda k: res[k]['graph_ms_median']
    res['launch_pair_us'] = round((g('views4') - g('views4_one_step')) / (a.iters - 1) * 1e3, 2) if a.iters > 1 else None
    res['floor_share'] = round(g('views4_floor') / g('views4'), 3)
    print(json.dumps(res))
    RC.emit(res, a.json)


if __name__ == '__main__':
    main()
