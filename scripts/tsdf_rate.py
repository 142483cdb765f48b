"""Rate of ops.tsdf_integrate and ops.tsdf_mesh (csrc/tsdf.hip) on the MI355X: tracks/s at 512 x 432, tl = 4, a lattice of `--res`
points along the longest side placed as data/mesh.py places it (profiles/tsdf_rate.md) - for the integration, for the extraction
and for both together -, the bytes every pass must move, and what that comes to against the rate of a plain device copy of the same
size measured in the same process (the yardstick of scripts/diag/stream_bw.py: (bytes read + bytes written) / time).

Each figure: `--warmup` untimed calls, then `--repeats` windows of `--calls` calls each, every window between two HIP events; the
median window gives the call time.  The caps of the mesh are given (found by one counting call) and a caller's workspace is passed,
so a call is its launches and the wrapper's allocations from torch's cache.  The same two calls captured once into a hipGraph and
replayed in the same windows give the time without the wrapper's host work.

Byte model (N = nx ny nz lattice points, C cells, V vertices, Q quads; what has to move if every array crossed the memory once per
launch that uses it - the tl gathers per lattice point go into depth maps of tl h w 4 bytes that are expected to stay in L2, the
rows of the stencil are read once per block from memory and again from LDS):
    integrate  reads  tl h w 4 (+ as much for the value)      writes N (4 + 1 + 4)
    flags      reads  N (4 + 1)                               writes N + N / 256 x 4
    quads      reads  N                                       writes N + N / 256 x 4
    scan       reads  2 N / 256 x 4                           writes 2 N / 256 x 4
    vertices   reads  N + V 8 (4 + 1 + 4)                     writes C 4 + V (12 + 12 + 4 + 1 + 4)
    faces      reads  N + Q (1 + 4 x 4)                       writes Q 2 x 12

    python scripts/tsdf_rate.py [--h 512 --w 432 --tl 4] [--res 256] [--warmup 3] [--repeats 9] [--calls 20] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rate_common as RC   # noqa: E402


def byte_model(tl, h, w, grid, vertices, quads, value=True):
    nx, ny, nz = grid
    N, C = nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)
    blocks = -(-N // 256)
    return {'integrate': tl * h * w * 4 * (2 if value else 1) + N * 9, 'flags': N * 5 + N + blocks * 4, 'quads': N + N + blocks * 4,
            'scan': blocks * 16, 'vertices': N + vertices * 72 + C * 4 + vertices * 33, 'faces': N + quads * 17 + quads * 24}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--trunc', type=float, default=3.0)
    RC.add_timing_args(ap, calls=20)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from depthinspace_amd.data import mesh as M
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    batch = synth.make_batch(st, 1, tl=a.tl, seed=7, scene='bumps', motion=0.1, with_primary=False, with_flow=False)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    disp, R, t, val = up(batch['disp0'][0, :, 0]), up(batch['R'][0]), up(batch['t'][0]), up(batch['ambient0'][0, :, 0])
    kept = ops.fuse_track(disp[None], R[None], t[None], st.K, st.baseline, val[None])
    m = int(kept['count'].sum().item())
    origin, voxel, trunc, grid = M.place_volume(kept['xyz'][:m], a.res, None, a.trunc)
    nx, ny, nz = grid
    integrate = lambda: ops.tsdf_integrate(disp, R, t, st.K, st.baseline, val, origin=origin, voxel=voxel, trunc=trunc, grid=grid)
    vol = integrate()
    nv, nf = (int(v) for v in ops.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, vcap=0, fcap=0)['count'].tolist())
    ws = torch.empty(lib.fn('dis_tsdf_mesh_workspace')(nx, ny, nz), dtype=torch.uint8, device='cuda')
    mesh = lambda v=vol: ops.tsdf_mesh(v[0], v[1], v[2], origin, voxel, vcap=nv, fcap=nf, workspace=ws)
    both = lambda: mesh(integrate())

    eager = lambda fn: RC.ms_fields('ms', RC.eager(fn, a.warmup, a.repeats, a.calls)[0])

    res = {'h': a.h, 'w': a.w, 'tl': a.tl, 'res': a.res, 'grid': list(grid), 'lattice_points': nx * ny * nz, 'voxel': voxel, 'trunc': trunc,
           'vertices': nv, 'triangles': nf, 'observed': round(float((vol[1] > 0).float().mean().item()), 4),
           'workspace_bytes': int(ws.numel())}
    model = byte_model(a.tl, a.h, a.w, grid, nv, nf // 2)
    res['model_bytes_by_launch'] = model
    groups = {'integrate': model['integrate'], 'mesh': sum(v for k, v in model.items() if k != 'integrate'), 'both': sum(model.values())}
    for name, fn in (('integrate', integrate), ('mesh', mesh), ('both', both)):
        e = eager(fn)
        gms, out = RC.replayed(fn, a.repeats, a.calls)
        g = RC.ms_fields('ms', gms)
        res[name] = {'call': e, 'tracks_per_s': round(1e3 / e['ms_median'], 1), 'graph': g, 'graph_tracks_per_s': round(1e3 / g['ms_median'], 1),
                     'model_bytes': groups[name], 'model_GB_per_s': round(groups[name] / g['ms_median'] / 1e6, 1)}
        if name == 'both':
            ref = mesh()
            torch.cuda.synchronize()
            res['graph_equals_eager'] = all(bool(torch.equal(out[k], ref[k])) for k in ref)
    # the yardstick: a device copy of as many bytes as the integration writes, and of the volume's 4-byte plane, in this process
    for name, nbytes in (('copy_9N', nx * ny * nz * 9), ('copy_4N', nx * ny * nz * 4)):
        x = torch.empty(nbytes // 4, dtype=torch.float32, device='cuda').normal_()
        y = torch.empty_like(x)
        w_ = eager(lambda: y.copy_(x))
        res[name] = {'bytes_moved': 2 * x.numel() * 4, 'ms_median': w_['ms_median'], 'GB_per_s': round(2 * x.numel() * 4 / w_['ms_median'] / 1e6, 1)}
    copy_rate = res['copy_9N']['GB_per_s']
    for name in ('integrate', 'mesh', 'both'):
        res[name]['share_of_copy_rate'] = round(res[name]['model_GB_per_s'] / copy_rate, 4)
    print(json.dumps(res))
    RC.emit(res, a.json)


if __name__ == '__main__':
    main()
