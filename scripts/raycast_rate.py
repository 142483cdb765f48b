"""Rate of ops.tsdf_raycast (csrc/raycast.hip) on the MI355X: tracks/s at 512 x 432, tl = 4 views (the track's own frames), a lattice of
`--res` points along the longest side placed and integrated as data/mesh.py does it, one track per call (profiles/raycast_rate.md) -
for variant 0 (a state byte per cell, dead bricks of 8 x 8 x 8 cells jumped over) and variant 1 (the plain march), whether the two give
the same bits, the share of dead bricks, and the time of the two pre-passes of variant 0, taken as a call of variant 0 with one view
of 2 x 2 pixels: the pre-passes do not depend on the views, and four rays are all that is left of the march.

Each figure: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  A caller's workspace is passed, so a call is its launches and the wrapper's three output
allocations from torch's cache.  The same call captured once into a hipGraph and replayed in the same windows gives the time without
the wrapper's host work.

    python scripts/raycast_rate.py [--h 512 --w 432 --tl 4] [--res 256] [--step 1.0] [--warmup 3] [--repeats 9] [--calls 20] [--json PATH]
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
    ap.add_argument('--step', type=float, default=1.0, help='in voxels')
    RC.add_timing_args(ap, calls=20)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from depthinspace_amd.data import mesh as M
    if not torch.cuda.is_available():
        raise SystemExit('raycast_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    batch = synth.make_batch(st, 1, tl=a.tl, seed=7, scene='bumps', motion=0.1, with_primary=False, with_flow=False)
    v = M.integrate_track(batch['disp0'][0, :, 0], batch['R'][0], batch['t'][0], batch['ambient0'][0, :, 0], st, a.res, None, a.trunc)
    nx, ny, nz = v['grid']
    step = float(np.float32(a.step * v['voxel']))
    ws = torch.empty(lib.fn('dis_tsdf_raycast_workspace')(nx, ny, nz), dtype=torch.uint8, device='cuda')

    def cast(variant, R=v['R'], t=v['t'], size=(a.h, a.w)):
        return ops.tsdf_raycast(v['tsdf'], v['weight'], v['vvalue'], v['origin'], v['voxel'], R, t, v['K'], st.baseline, size=size, step=step,
                                workspace=ws, variant=variant)

    out0, out1 = cast(0), cast(1)
    torch.cuda.synchronize()
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    nb = -(-(nx - 1) // 8) * -(-(ny - 1) // 8) * -(-(nz - 1) // 8)
    off = -(-cells // 16) * 16
    cast(0)
    torch.cuda.synchronize()
    bricks, state = ws[off:off + 4 * nb].view(torch.int32), ws[:cells]
    res = {'h': a.h, 'w': a.w, 'views': a.tl, 'res': a.res, 'grid': [nx, ny, nz], 'lattice_points': nx * ny * nz, 'voxel': v['voxel'],
           'step_voxels': a.step, 'hit': round(float((out0['disp'] > 0).float().mean().item()), 4),
           'variants_equal_bits': all(bool(torch.equal(out0[k].view(torch.int32), out1[k].view(torch.int32))) for k in out0),
           'bricks': nb, 'dead_brick_share': round(float((bricks == 0).float().mean().item()), 4),
           'cell_state_share': [round(float((state == s).float().mean().item()), 4) for s in (0, 1, 2)], 'workspace_bytes': int(ws.numel())}
    for name, fn in (('variant0', lambda: cast(0)), ('variant1', lambda: cast(1)),
                     ('prepasses', lambda: cast(0, v['R'][:1], v['t'][:1], (2, 2)))):
        ms, gms, _, _ = RC.time_call(fn, a.warmup, a.repeats, a.calls)
        res[name] = RC.timing_fields(1, ms, gms)
    res['speedup_graph'] = round(res['variant1']['graph_ms_median'] / res['variant0']['graph_ms_median'], 3)
    print(json.dumps(res))
    RC.emit(res, a.json)


if __name__ == '__main__':
    main()
