"""Track fusion: the per-frame disparity maps of every track of a dataset root -> one point cloud per track, and a cross-view
consistency report that needs no ground truth.

For every track directory the chosen disparities - `disp` (gt) or `sgm_disp` (sgm) of frames.npz, or the `disp` of
single_frame_disp.npz / multi_frame_disp.npz - go with the stored poses R, t and the K and baseline of settings.npz through
ops.fuse_track (include/dis_hip.h, section "track fusion"): every pixel is lifted to world coordinates, checked against the depth of
the other frames, averaged with the agreeing samples and kept once, by the lowest-index frame that sees its surface.  The cloud is written
as <track>/fused_<disp>.ply (data/ply.py: x y z, normal, the ambient intensity, the number of agreeing views); nothing else is touched.

    python -m depthinspace_amd.data.fuse ROOT [--disp gt|sgm|single_frame|multi_frame] [--tol T] [--min-views N] [--force] [--report]

A track whose cloud exists is skipped unless --force is given.  --report also fuses the tracks that are skipped and prints, over the
dataset: the share of valid pixels, the share of the (pixel, other frame) pairs in which the pixel is seen, the consistent share of
those, the mean residual of the seen pixels, the points kept - and, where frames.npz stores a ground-truth `disp` and the source is
another one, the mean distance of the kept points from the ground-truth point of their pixel, relative to that point's depth.
"""
import argparse
import os

import numpy as np
import torch

from . import packed, ply
from .dataset import load_settings
from .trackfiles import SOURCES, load_track, report_text


def fuse_arrays(disp, R, t, value, settings, tol=0.01, min_views=2, device='cuda'):
    """one track, float32 numpy in, through ops.fuse_track -> dict of numpy arrays: xyz, normal (m, 3), value (m), src (m), views (m)
    uint8 of the m kept pixels and the dense maps views, seen, keep, resid (tl, H, W)"""
    from .. import ops
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)[None]).to(dev)
    r = ops.fuse_track(up(disp), up(R), up(t), np.asarray(settings.K, dtype=np.float32), settings.baseline,
                       None if value is None else up(value), tol=tol, min_views=min_views, want_dense=True)
    m = int(r['count'].sum().item())
    out = {k: r[k][:m].cpu().numpy() for k in ('xyz', 'normal', 'value', 'src')}
    for k in ('views', 'seen', 'keep', 'resid'):
        out[k + '_map'] = r[k][0].cpu().numpy()
    out['views'] = out['views_map'].reshape(-1)[out['src']]
    return out


def gt_points(gt, R, t, settings, src):
    """the ground-truth world points of the pixels `src` (linear indices into (tl, H, W)) and their depths, float64"""
    tl, H, W = gt.shape
    K = np.asarray(settings.K, dtype=np.float64)
    i, v, u = src // (H * W), (src // W) % H, src % W
    with np.errstate(divide='ignore', invalid='ignore'):
        z = K[0, 0] * float(settings.baseline) / gt.astype(np.float64)[i, v, u]
    P = np.stack([z * (u - K[0, 2]) / K[0, 0], z * (v - K[1, 2]) / K[1, 1], z], 1)
    Xw = np.einsum('mji,mj->mi', R.astype(np.float64)[i], P - t.astype(np.float64)[i])
    return Xw, z


def fuse_dataset(data_root, source='multi_frame', tol=0.01, min_views=2, force=False, report=False, device='cuda'):
    """Writes <track>/fused_<source>.ply for every track directory of data_root that has none (force: for all of them), each through a
    temporary file; frames.npz and everything else stay as they are.  Returns the number of clouds written.  report=True: every track
    is fused, whether its cloud is written or not, and the return value is a dict - valid, seen, consistent (shares), resid (mean over
    the seen pixels), points, tracks, written and, where it can be measured, gt_distance - printed as one line."""
    data_root = str(data_root)
    settings = load_settings(data_root)
    done = 0
    acc = dict(pixels=0, valid=0, pairs=0, seen=0, cons=0, seen_px=0, resid=0.0, points=0, tracks=0, gt_sum=0.0, gt_n=0)
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, f'fused_{source}.ply')
        write = force or not os.path.exists(path)
        if not (write or report):
            continue
        disp, R, t, amb, gt = load_track(d, source)
        r = fuse_arrays(disp, R, t, amb, settings, tol, min_views, device)
        if write:
            ply.write_ply(path, r['xyz'], r['normal'], r['value'], r['views'],
                          comments=(f'fused from {source} disparities, tol {tol:g}, min_views {min_views}',))
            done += 1
        if not report:
            continue
        tl = disp.shape[0]
        views, seen = r['views_map'].astype(np.int64), r['seen_map'].astype(np.int64)
        acc['pixels'] += views.size
        acc['valid'] += int((views > 0).sum())
        acc['pairs'] += int((views > 0).sum()) * (tl - 1)
        acc['seen'] += int(seen.sum())
        acc['cons'] += int(np.maximum(views - 1, 0).sum())
        acc['seen_px'] += int((seen > 0).sum())
        acc['resid'] += float(r['resid_map'].astype(np.float64)[seen > 0].sum())
        acc['points'] += len(r['src'])
        acc['tracks'] += 1
        if gt is not None and source != 'gt' and len(r['src']):
            Xw, z = gt_points(gt, R, t, settings, r['src'].astype(np.int64))
            ok = np.isfinite(z) & (z > 0)
            dist = np.linalg.norm(r['xyz'].astype(np.float64) - Xw, axis=1)
            acc['gt_sum'] += float((dist[ok] / z[ok]).sum())
            acc['gt_n'] += int(ok.sum())
    if not report:
        return done
    div = lambda a, b: a / b if b else float('nan')
    res = {'valid': div(acc['valid'], acc['pixels']), 'seen': div(acc['seen'], acc['pairs']), 'consistent': div(acc['cons'], acc['seen']),
           'resid': div(acc['resid'], acc['seen_px']), 'points': acc['points'], 'tracks': acc['tracks'], 'written': done}
    if acc['gt_n']:
        res['gt_distance'] = acc['gt_sum'] / acc['gt_n']
    print(f'fusion of the {source} disparities over {data_root} (tol {tol:g}, min_views {min_views}): '
          + report_text(res, '.6f'))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.fuse', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('root')
    ap.add_argument('--disp', default='multi_frame', choices=SOURCES, help='which disparities are fused')
    ap.add_argument('--tol', type=float, default=0.01, help='relative depth tolerance of the cross-view check, in (0, 1)')
    ap.add_argument('--min-views', type=int, default=2, help='a point is kept when this many frames agree on it, its own included')
    ap.add_argument('--force', action='store_true', help='also rewrite the clouds that exist')
    ap.add_argument('--report', action='store_true', help='also print the consistency figures over the dataset')
    a = ap.parse_args(argv)
    r = fuse_dataset(a.root, a.disp, a.tol, a.min_views, force=a.force, report=a.report)
    print(f'{r["written"] if a.report else r} clouds written under {a.root}')


if __name__ == '__main__':
    main()
