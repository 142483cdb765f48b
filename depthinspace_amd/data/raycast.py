"""Volumetric fusion read back: the per-frame disparity maps of every track of a dataset root -> the fused surface as one disparity
map, one normal map and one intensity map per frame.

For every track directory the chosen disparities - `disp` (gt) or `sgm_disp` (sgm) of frames.npz, or the `disp` of
single_frame_disp.npz / multi_frame_disp.npz - are placed and integrated exactly as data/mesh.py does it (mesh.integrate_track: the
lattice around the points ops.fuse_track keeps, ops.tsdf_integrate), and the volume is then cast into the track's own frames by
ops.tsdf_raycast (include/dis_hip.h, section "volumetric fusion"): per pixel the first crossing of the trilinear tsdf from observed free
space into the surface.  The maps are written as <track>/raycast_<disp>.npz with `disp` (tl, 1, H, W) - the key and shape of
multi_frame_disp.npz -, `normal` (tl, 3, H, W), world axes, towards free space, and `value` (tl, 1, H, W), float32; a pixel whose ray
meets no surface is 0 in all three.  Nothing else is touched.

    python -m depthinspace_amd.data.raycast ROOT [--disp gt|sgm|single_frame|multi_frame] [--res N | --voxel V] [--trunc VOXELS]
                                            [--min-weight N] [--step VOXELS] [--tol T] [--min-views N] [--force] [--report]

--res, --voxel, --trunc, --min-weight, --tol, --min-views: as in data/mesh.py.  --step: the distance between two samples of a ray, in
voxels (default 1; 1 / 8 .. 8).  A track without a cross-view consistent point is reported and skipped; a track whose file exists is
skipped unless --force is given.  --report also casts the tracks that are skipped and prints, over the dataset: tracks and files
written; hit, the share of pixels with a surface; kept, the share of input-valid pixels that are hit; moved, the mean
|raycast - input| / input over the pixels valid in both (how far fusion moves what went in) - and, where frames.npz stores a
ground-truth `disp` and the source is another one, err_in and err_out, the mean |d - gt| / gt of the input and of the raycast over the
pixels valid in all three.
"""
import argparse
import os

import numpy as np

from . import packed
from .dataset import load_settings
from .mesh import integrate_track
from .trackfiles import SOURCES, load_track, report_text, write_npz


def raycast_arrays(disp, R, t, value, settings, res=256, voxel=None, trunc_voxels=3.0, min_weight=1, step_voxels=1.0, tol=0.01, min_views=2,
                   device='cuda'):
    """one track, float32 numpy in, through mesh.integrate_track and ops.tsdf_raycast into the track's own frames -> dict of numpy
    arrays disp (tl, 1, H, W), normal (tl, 3, H, W), value (tl, 1, H, W) float32, and origin, voxel, trunc, grid, step - or None when
    fuse_track keeps no point"""
    from .. import ops
    v = integrate_track(disp, R, t, value, settings, res, voxel, trunc_voxels, tol, min_views, device)
    if v is None:
        return None
    step = float(np.float32(float(step_voxels) * v['voxel']))
    g = ops.tsdf_raycast(v['tsdf'], v['weight'], v['vvalue'], v['origin'], v['voxel'], v['R'], v['t'], v['K'], settings.baseline,
                         size=disp.shape[-2:], step=step, min_weight=min_weight)
    out = {'disp': g['disp'][:, None].cpu().numpy(), 'normal': g['normal'].cpu().numpy(), 'value': g['value'][:, None].cpu().numpy()}
    out.update(origin=v['origin'], voxel=v['voxel'], trunc=v['trunc'], grid=v['grid'], step=step)
    return out


def _valid(d):
    return np.isfinite(d) & (d > 0)


def raycast_dataset(data_root, source='multi_frame', res=256, voxel=None, trunc_voxels=3.0, min_weight=1, step_voxels=1.0, tol=0.01,
                    min_views=2, force=False, report=False, device='cuda'):
    """Writes <track>/raycast_<source>.npz for every track directory of data_root that has none (force: for all of them), each through
    a temporary file; frames.npz and everything else stay as they are.  Returns the number of files written.  report=True: every track
    is cast, whether its file is written or not, and the return value is a dict - tracks, written, hit, kept, moved and, where they can
    be measured, err_in and err_out - printed as one line."""
    data_root = str(data_root)
    settings = load_settings(data_root)
    done = 0
    acc = dict(tracks=0, pixels=0, hit=0, valid_in=0, kept=0, moved=0.0, gt_n=0, err_in=0.0, err_out=0.0)
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, f'raycast_{source}.npz')
        write = force or not os.path.exists(path)
        if not (write or report):
            continue
        disp, R, t, amb, gt = load_track(d, source)
        r = raycast_arrays(disp, R, t, amb, settings, res, voxel, trunc_voxels, min_weight, step_voxels, tol, min_views, device)
        acc['tracks'] += 1
        if r is None:
            print(f'{d}: no cross-view consistent point to place the volume around (tol {tol:g}, min_views {min_views}); skipped')
            continue
        if write:
            write_npz(path, {k: r[k] for k in ('disp', 'normal', 'value')})
            done += 1
        if not report:
            continue
        out = r['disp'][:, 0].astype(np.float64)
        inp = disp.astype(np.float64)
        hit, ok = out > 0, _valid(disp)
        both = hit & ok
        acc['pixels'] += hit.size
        acc['hit'] += int(hit.sum())
        acc['valid_in'] += int(ok.sum())
        acc['kept'] += int(both.sum())
        acc['moved'] += float((np.abs(out[both] - inp[both]) / inp[both]).sum())
        if gt is not None and source != 'gt':
            m = both & _valid(gt)
            g = gt.astype(np.float64)[m]
            acc['gt_n'] += int(m.sum())
            acc['err_in'] += float((np.abs(inp[m] - g) / g).sum())
            acc['err_out'] += float((np.abs(out[m] - g) / g).sum())
    if not report:
        return done
    div = lambda a, b: a / b if b else float('nan')
    res_ = {'tracks': acc['tracks'], 'written': done, 'hit': div(acc['hit'], acc['pixels']), 'kept': div(acc['kept'], acc['valid_in']),
            'moved': div(acc['moved'], acc['kept'])}
    if acc['gt_n']:
        res_['err_in'] = acc['err_in'] / acc['gt_n']
        res_['err_out'] = acc['err_out'] / acc['gt_n']
    print(f'raycast of the {source} disparities over {data_root} (trunc {trunc_voxels:g} voxels, min_weight {min_weight}, step '
          f'{step_voxels:g} voxels): ' + report_text(res_, '.6f'))
    return res_


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.raycast', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('root')
    ap.add_argument('--disp', default='multi_frame', choices=SOURCES, help='which disparities are integrated')
    size = ap.add_mutually_exclusive_group()
    size.add_argument('--res', type=int, default=256, help='lattice points along the longest side of the padded box')
    size.add_argument('--voxel', type=float, default=None, help='the lattice spacing, instead of --res')
    ap.add_argument('--trunc', type=float, default=3.0, help='the truncation distance in voxels')
    ap.add_argument('--min-weight', type=int, default=1, help='frames that must observe each of the eight lattice points of a sample')
    ap.add_argument('--step', type=float, default=1.0, help='the distance between two samples of a ray, in voxels')
    ap.add_argument('--tol', type=float, default=0.01, help='relative depth tolerance of the cross-view check that places the volume')
    ap.add_argument('--min-views', type=int, default=2, help='agreeing frames a point needs to count for the placement')
    ap.add_argument('--force', action='store_true', help='also rewrite the files that exist')
    ap.add_argument('--report', action='store_true', help='also print the raycast figures over the dataset')
    a = ap.parse_args(argv)
    if a.voxel is not None and not a.voxel > 0:
        ap.error('--voxel must be positive')
    if not a.trunc > 0:
        ap.error('--trunc must be positive')
    if not 0.125 <= a.step <= 8:
        ap.error('--step must lie in 1 / 8 .. 8 voxels')
    r = raycast_dataset(a.root, a.disp, a.res, a.voxel, a.trunc, a.min_weight, a.step, a.tol, a.min_views, force=a.force, report=a.report)
    print(f'{r["written"] if a.report else r} raycast files written under {a.root}')


if __name__ == '__main__':
    main()
