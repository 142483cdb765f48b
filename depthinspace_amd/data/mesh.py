"""Volumetric fusion: the per-frame disparity maps of every track of a dataset root -> one triangle mesh per track.

For every track directory the chosen disparities - `disp` (gt) or `sgm_disp` (sgm) of frames.npz, or the `disp` of
single_frame_disp.npz / multi_frame_disp.npz - go with the stored poses R, t and the K and baseline of settings.npz through
ops.tsdf_integrate and ops.tsdf_mesh (include/dis_hip.h, section "volumetric fusion"): every point of a regular lattice is projected
into every frame, the truncated signed distances to the frames' surfaces are averaged, and naive surface nets turn the zero crossing
into shared vertices and triangles.  Unlike the cloud of data/fuse.py the surface averages the frames, and it has connectivity.  The
volume is placed around the points ops.fuse_track keeps - the cross-view consistent ones, so a stray disparity cannot blow the box up -,
padded by trunc + voxel.  The mesh is written as <track>/mesh_<disp>.ply (data/ply.py: x y z, normal, the ambient intensity, the
smallest number of frames over the vertex's eight lattice points; triangles); nothing else is touched.

    python -m depthinspace_amd.data.mesh ROOT [--disp gt|sgm|single_frame|multi_frame] [--res N | --voxel V] [--trunc VOXELS]
                                         [--min-weight N] [--tol T] [--min-views N] [--force] [--report]

--res: lattice points along the longest side of the padded box (default 256); --voxel: the lattice spacing instead, in the units of
the baseline.  Every extent is clamped to 1024 points.  --trunc: the truncation distance in voxels (default 3).  --min-weight: a cell
carries a vertex only when each of its eight lattice points was observed by that many frames (default 1).  --tol, --min-views: the
cross-view check that selects the points the box is placed around.  A track without such a point is reported and skipped; a track
whose mesh exists is skipped unless --force is given.  --report also meshes the tracks that are skipped and prints, over the dataset:
tracks and meshes written, vertices and triangles, the share of lattice points observed by a frame, boundary edges (undirected edges
with one triangle) per triangle, the surface area - and, where frames.npz stores a ground-truth `disp` and the source is another one,
the mean |depth_gt - z| / z of the vertices over the frames in which they project onto a valid ground-truth pixel.
"""
import argparse
import os

import numpy as np
import torch

from . import packed, ply
from .dataset import load_settings
from .trackfiles import SOURCES, load_track, report_text

MAX_EXTENT = 1024


def place_volume(points, res=256, voxel=None, trunc_voxels=3.0):
    """the lattice around `points` (m, 3), a device tensor with m > 0: their bounding box (min and max taken on the device) padded by
    trunc + voxel on every side.  voxel None: `res` lattice points along the longest padded side.  -> origin (3) float32, voxel, trunc
    (floats, exact in float32), grid (nx, ny, nz), every extent in 2 .. 1024 - or None when the box has no extent to size a voxel from"""
    box = torch.stack([points.min(dim=0).values, points.max(dim=0).values]).double().cpu().numpy()
    lo, hi = box[0], box[1]
    pad_voxels = float(trunc_voxels) + 1.0
    if voxel is None:
        inner = int(res) - 1 - 2.0 * pad_voxels
        if inner < 1:
            raise ValueError(f'--res {res} leaves no lattice point inside a padding of {pad_voxels:g} voxels per side')
        voxel = float((hi - lo).max()) / inner
    voxel = float(np.float32(voxel))
    if not (np.isfinite(voxel) and voxel > 0 and np.isfinite(box).all()):
        return None
    trunc = float(np.float32(float(trunc_voxels) * voxel))
    origin = (lo - (trunc + voxel)).astype(np.float32)
    top = hi + (trunc + voxel)
    grid = tuple(int(min(MAX_EXTENT, max(2, np.ceil((top[k] - float(origin[k])) / voxel - 1e-4) + 1))) for k in range(3))
    return origin, voxel, trunc, grid


def _upload(disp, R, t, value, device):
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return up(disp), up(R), up(t), None if value is None else up(value)


def place_track(disp, R, t, value, settings, res=256, voxel=None, trunc_voxels=3.0, tol=0.01, min_views=2, device='cuda'):
    """one track, float32 numpy in: the lattice placed around the points ops.fuse_track keeps (place_volume) -> origin, voxel, trunc, grid
    - or None when fuse_track keeps no point or the box has no extent.  The first half of integrate_track"""
    from .. import ops
    d_disp, d_R, d_t, d_val = _upload(disp, R, t, value, device)
    r = ops.fuse_track(d_disp[None], d_R[None], d_t[None], np.asarray(settings.K, dtype=np.float32), settings.baseline,
                       None if d_val is None else d_val[None], tol=tol, min_views=min_views)
    m = int(r['count'].sum().item())
    if m == 0:
        return None
    return place_volume(r['xyz'][:m], res, voxel, trunc_voxels)


def integrate_placed(disp, R, t, value, settings, place, device='cuda'):
    """one track (or some of its frames), float32 numpy in, integrated by ops.tsdf_integrate into the lattice `place` = origin, voxel,
    trunc, grid of place_track: the second half of integrate_track.  -> its dict"""
    from .. import ops
    d_disp, d_R, d_t, d_val = _upload(disp, R, t, value, device)
    K = np.asarray(settings.K, dtype=np.float32)
    origin, vx, trunc, grid = place
    tsdf, weight, vvalue = ops.tsdf_integrate(d_disp, d_R, d_t, K, settings.baseline, d_val, origin=origin, voxel=vx, trunc=trunc, grid=grid)
    return dict(tsdf=tsdf, weight=weight, vvalue=vvalue, R=d_R, t=d_t, origin=origin, voxel=vx, trunc=trunc, grid=grid, K=K)


def integrate_track(disp, R, t, value, settings, res=256, voxel=None, trunc_voxels=3.0, tol=0.01, min_views=2, device='cuda'):
    """one track, float32 numpy in: the volume placed around the points ops.fuse_track keeps (place_track) and integrated by
    ops.tsdf_integrate (integrate_placed) - what data/mesh.py and data/raycast.py share.  -> dict of the device tensors tsdf, weight,
    vvalue, R, t and origin, voxel, trunc, grid, K - or None when fuse_track keeps no point or the box has no extent"""
    place = place_track(disp, R, t, value, settings, res, voxel, trunc_voxels, tol, min_views, device)
    if place is None:
        return None
    return integrate_placed(disp, R, t, value, settings, place, device)


def mesh_arrays(disp, R, t, value, settings, res=256, voxel=None, trunc_voxels=3.0, min_weight=1, tol=0.01, min_views=2, device='cuda'):
    """one track, float32 numpy in, through integrate_track (the placement by ops.fuse_track, ops.tsdf_integrate) and ops.tsdf_mesh ->
    dict of numpy arrays xyz, normal (V, 3), value (V), views (V) uint8, faces (M, 3) int32, and origin, voxel, trunc, grid, observed
    (the share of lattice points with weight > 0) - or None when fuse_track keeps no point"""
    from .. import ops
    v = integrate_track(disp, R, t, value, settings, res, voxel, trunc_voxels, tol, min_views, device)
    if v is None:
        return None
    g = ops.tsdf_mesh(v['tsdf'], v['weight'], v['vvalue'], v['origin'], v['voxel'], min_weight=min_weight)
    out = {k: g[k].cpu().numpy() for k in ('xyz', 'normal', 'value', 'views', 'faces')}
    out.update(origin=v['origin'], voxel=v['voxel'], trunc=v['trunc'], grid=v['grid'],
               observed=float((v['weight'] > 0).float().mean().item()))
    return out


def mesh_stats(xyz, faces):
    """-> (boundary edges: undirected edges that belong to one triangle only, surface area), in float64 on the host"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(faces):
        return 0, 0.0
    xyz = np.asarray(xyz, dtype=np.float64)
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e[:, 0] * len(xyz) + e[:, 1], return_counts=True)
    tn = np.cross(xyz[faces[:, 1]] - xyz[faces[:, 0]], xyz[faces[:, 2]] - xyz[faces[:, 0]])
    return int((counts == 1).sum()), float(0.5 * np.linalg.norm(tn, axis=1).sum())


def gt_depth_error(xyz, gt, R, t, settings):
    """-> (sum, number) of |depth_gt - z| / z over the (vertex, frame) pairs in which the vertex projects onto a valid ground-truth
    pixel (the nearest one), float64 on the host"""
    tl, H, W = gt.shape
    K = np.asarray(settings.K, dtype=np.float64)
    fb = K[0, 0] * float(settings.baseline)
    X = np.asarray(xyz, dtype=np.float64)
    total, number = 0.0, 0
    with np.errstate(all='ignore'):
        for f in range(tl):
            Xc = X @ R[f].astype(np.float64).T + t[f].astype(np.float64)
            z = Xc[:, 2]
            u, v = np.floor(K[0, 0] * Xc[:, 0] / z + K[0, 2] + 0.5), np.floor(K[1, 1] * Xc[:, 1] / z + K[1, 2] + 0.5)
            ok = (z > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            d = gt[f][np.where(ok, v, 0).astype(np.int64), np.where(ok, u, 0).astype(np.int64)].astype(np.float64)
            ok &= np.isfinite(d) & (d > 0)
            total += float((np.abs(fb / d[ok] - z[ok]) / z[ok]).sum())
            number += int(ok.sum())
    return total, number


def mesh_dataset(data_root, source='multi_frame', res=256, voxel=None, trunc_voxels=3.0, min_weight=1, tol=0.01, min_views=2, force=False,
                 report=False, device='cuda'):
    """Writes <track>/mesh_<source>.ply for every track directory of data_root that has none (force: for all of them), each through a
    temporary file; frames.npz and everything else stay as they are.  Returns the number of meshes written.  report=True: every track
    is meshed, whether its file is written or not, and the return value is a dict - tracks, written, vertices, triangles, observed,
    boundary (edges per triangle), area and, where it can be measured, gt_depth_error - printed as one line."""
    data_root = str(data_root)
    settings = load_settings(data_root)
    done = 0
    acc = dict(tracks=0, vertices=0, triangles=0, lattice=0, observed=0.0, boundary=0, area=0.0, gt_sum=0.0, gt_n=0)
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, f'mesh_{source}.ply')
        write = force or not os.path.exists(path)
        if not (write or report):
            continue
        disp, R, t, amb, gt = load_track(d, source)
        r = mesh_arrays(disp, R, t, amb, settings, res, voxel, trunc_voxels, min_weight, tol, min_views, device)
        acc['tracks'] += 1
        if r is None:
            print(f'{d}: no cross-view consistent point to place the volume around (tol {tol:g}, min_views {min_views}); skipped')
            continue
        if write:
            nx, ny, nz = r['grid']
            ply.write_mesh(path, r['xyz'], r['normal'], r['value'], r['views'], r['faces'],
                           comments=(f'surface nets of the {source} disparities, lattice {nx} x {ny} x {nz}, voxel {r["voxel"]:g}, '
                                     f'trunc {r["trunc"]:g}, min_weight {min_weight}',))
            done += 1
        if not report:
            continue
        points = int(np.prod(r['grid']))
        boundary, area = mesh_stats(r['xyz'], r['faces'])
        acc['vertices'] += len(r['xyz'])
        acc['triangles'] += len(r['faces'])
        acc['lattice'] += points
        acc['observed'] += r['observed'] * points
        acc['boundary'] += boundary
        acc['area'] += area
        if gt is not None and source != 'gt' and len(r['xyz']):
            s, k = gt_depth_error(r['xyz'], gt, R, t, settings)
            acc['gt_sum'] += s
            acc['gt_n'] += k
    if not report:
        return done
    div = lambda a, b: a / b if b else float('nan')
    res_ = {'tracks': acc['tracks'], 'written': done, 'vertices': acc['vertices'], 'triangles': acc['triangles'],
            'observed': div(acc['observed'], acc['lattice']), 'boundary': div(acc['boundary'], acc['triangles']), 'area': acc['area']}
    if acc['gt_n']:
        res_['gt_depth_error'] = acc['gt_sum'] / acc['gt_n']
    print(f'meshes of the {source} disparities over {data_root} (trunc {trunc_voxels:g} voxels, min_weight {min_weight}): '
          + report_text(res_, '.6f'))
    return res_


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.mesh', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('root')
    ap.add_argument('--disp', default='multi_frame', choices=SOURCES, help='which disparities are integrated')
    size = ap.add_mutually_exclusive_group()
    size.add_argument('--res', type=int, default=256, help='lattice points along the longest side of the padded box')
    size.add_argument('--voxel', type=float, default=None, help='the lattice spacing, instead of --res')
    ap.add_argument('--trunc', type=float, default=3.0, help='the truncation distance in voxels')
    ap.add_argument('--min-weight', type=int, default=1, help='frames that must observe each of the eight lattice points of a vertex')
    ap.add_argument('--tol', type=float, default=0.01, help='relative depth tolerance of the cross-view check that places the volume')
    ap.add_argument('--min-views', type=int, default=2, help='agreeing frames a point needs to count for the placement')
    ap.add_argument('--force', action='store_true', help='also rewrite the meshes that exist')
    ap.add_argument('--report', action='store_true', help='also print the mesh figures over the dataset')
    a = ap.parse_args(argv)
    if a.voxel is not None and not a.voxel > 0:
        ap.error('--voxel must be positive')
    if not a.trunc > 0:
        ap.error('--trunc must be positive')
    r = mesh_dataset(a.root, a.disp, a.res, a.voxel, a.trunc, a.min_weight, a.tol, a.min_views, force=a.force, report=a.report)
    print(f'{r["written"] if a.report else r} meshes written under {a.root}')


if __name__ == '__main__':
    main()
