"""Optical-flow presave: the `flow.npz` that multi-frame training reads (feature warps, forward-backward masks, flow consistency).

For every track directory of a dataset root that has no flow.npz, the frames of frames.npz are matched pairwise with ops.dense_flow - a
coarse-to-fine Horn-Schunck flow with warping on the device (include/dis_hip.h, section "dense optical flow") - and flow.npz is written
with flow_ij (1, 2, H, W) for the ordered pairs i != j: where pixel p of frame i lies in frame j, minus p, channel 0 along x.  The
reference takes these arrays from an external LiteFlowNet fork and says that any flow estimator may be substituted; this is not
LiteFlowNet and does not try to be: it is dense, smooth, blind to occlusion and limited to motions its pyramid covers.

The flows come from the `ambient` frames by default.  The dot pattern in `im` is fixed to the projector, not to the surface: it moves
over the scene with the camera and breaks the brightness constancy the method rests on; --source im is there for tracks without a usable
ambient image.  Each frame is normalised by its own mean and deviation, so exposure changes between the frames do not matter.

    python -m depthinspace_amd.data.presave_flow ROOT [--source ambient|im|geometry] [--alpha A] [--warps N] [--iters N] [--min-size N]
                                                      [--disp gt|sgm|single_frame|multi_frame] [--tol T] [--force] [--report] [--pack]

--report compares the estimate with the flow.npz already there (rendered and synthetic tracks carry exact flows) and writes nothing.

--source geometry reads no image: the flow is the one that the chosen disparities (--disp) and the poses R, t stored in frames.npz imply
(ops.rigid_flow; include/dis_hip.h, section "disparity alignment") - for tracks whose poses come from data/presave_pose.py --pairwise
disp, so that the chain disparity -> poses -> flow.npz -> multi-frame training needs no image-based flow.  It holds for a static scene
only; a pixel without a valid disparity, or whose point lies behind the other camera, gets a zero flow; its accuracy is that of the
disparities and the poses.  With --report it prints the end-point error against the stored flows over the pixels that pass the depth
test of frame j (--tol, relative, as in data/fuse.py), the share of those pixels (`visible`) and the share written as zeros (`zeros`).
"""
import argparse
import os

import numpy as np
import torch

from . import packed
from .trackfiles import report_text, write_npz

REPORT_THRESHOLDS = (0.5, 1, 2)


def pair_keys(tl):
    return [(i, j) for i in range(tl) for j in range(tl) if i != j]


def estimate_flows(frames, alpha=1.0, warps=3, iters=64, min_size=8, device='cuda'):
    """frames (tl, 1, H, W) or (tl, H, W) float32 numpy -> {'flow_ij': (1, 2, H, W) float32 numpy} for the ordered pairs i != j
    (ops.dense_flow on the device)"""
    from .. import ops
    fr = np.ascontiguousarray(frames, dtype=np.float32)
    fr = fr.reshape((1, fr.shape[0]) + fr.shape[-2:])
    tl = fr.shape[1]
    flow = ops.dense_flow(torch.from_numpy(fr).to(torch.device(device)), alpha, warps, iters, min_size).cpu().numpy()
    return {f'flow_{i}{j}': np.ascontiguousarray(flow[:, i * tl + j]) for i, j in pair_keys(tl)}


def geometry_flows(d, disp_source, settings, tol=0.01, device='cuda'):
    """one track directory: the flows that its `disp_source` disparities and the R, t of its frames.npz imply (ops.rigid_flow on the
    device) -> ({'flow_ij': (1, 2, H, W) float32 numpy}, {'flow_ij': (1, H, W) bool: the pixel passes the depth test in frame j})"""
    from .. import ops
    from .trackfiles import load_disp
    with np.load(os.path.join(d, 'frames.npz')) as f:
        if 'R' not in f.files or 't' not in f.files:
            raise ValueError(f'{d}/frames.npz stores no poses R, t (data/presave_pose.py writes them)')
        R, t = np.asarray(f['R'], dtype=np.float32), np.asarray(f['t'], dtype=np.float32)
    disp = load_disp(d, disp_source)
    tl = disp.shape[0]
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a[None], dtype=np.float32)).to(dev)
    flow, vis = ops.rigid_flow(up(disp), up(R), up(t), np.asarray(settings.K, dtype=np.float32), settings.baseline, tol=tol, want_visible=True)
    flow, vis = flow.cpu().numpy(), vis.cpu().numpy()
    return ({f'flow_{i}{j}': np.ascontiguousarray(flow[:, i * tl + j]) for i, j in pair_keys(tl)},
            {f'flow_{i}{j}': vis[:, i * tl + j] != 0 for i, j in pair_keys(tl)})


def geometry_report(data_root, disp_source='gt', tol=0.01, device='cuda'):
    """flow_report for --source geometry: `epe` and the `under*` fractions over the visible pixels, `visible` their share of all pixels
    of all pairs, `zeros` the share of pixels written as a zero flow.  Writes nothing."""
    from .dataset import load_settings
    settings = load_settings(data_root)
    total, count, pixels, zeros = 0.0, 0, 0, 0
    under = [0] * len(REPORT_THRESHOLDS)
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, 'flow.npz')
        if not os.path.exists(path):
            raise ValueError(f'{d}: --report needs a flow.npz to compare with')
        est, vis = geometry_flows(d, disp_source, settings, tol, device)
        with np.load(path) as f:
            for k, e in est.items():
                err = np.sqrt(((e.astype(np.float64) - f[k].astype(np.float64)) ** 2).sum(axis=1))
                pixels += err.size
                zeros += int(((e[:, 0] == 0) & (e[:, 1] == 0)).sum())
                err = err[vis[k]]
                total += float(err.sum())
                count += err.size
                for n_, t in enumerate(REPORT_THRESHOLDS):
                    under[n_] += int((err < t).sum())
    res = {'epe': total / count if count else float('nan')}
    for n_, t in enumerate(REPORT_THRESHOLDS):
        res[f'under{t}'] = under[n_] / count if count else float('nan')
    res['visible'] = count / pixels if pixels else float('nan')
    res['zeros'] = zeros / pixels if pixels else float('nan')
    return res


def _frames_of(d, source):
    with np.load(os.path.join(d, 'frames.npz')) as f:
        if source not in f.files:
            raise ValueError(f'{d}/frames.npz has no array `{source}`')
        return f[source]


def flow_report(data_root, source='ambient', alpha=1.0, warps=3, iters=64, min_size=8, device='cuda'):
    """The estimate against the flows stored in every track's flow.npz: mean end-point error in pixels (`epe`) and the fraction of
    pixels whose end-point error is under 0.5, 1 and 2 px (`under0.5`, `under1`, `under2`), over all pairs of all tracks of data_root.
    Writes nothing."""
    total, count = 0.0, 0
    under = [0] * len(REPORT_THRESHOLDS)
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, 'flow.npz')
        if not os.path.exists(path):
            raise ValueError(f'{d}: --report needs a flow.npz to compare with')
        est = estimate_flows(_frames_of(d, source), alpha, warps, iters, min_size, device)
        with np.load(path) as f:
            for k, e in est.items():
                err = np.sqrt(((e.astype(np.float64) - f[k].astype(np.float64)) ** 2).sum(axis=1))
                total += float(err.sum())
                count += err.size
                for n_, t in enumerate(REPORT_THRESHOLDS):
                    under[n_] += int((err < t).sum())
    res = {'epe': total / count if count else float('nan')}
    for n_, t in enumerate(REPORT_THRESHOLDS):
        res[f'under{t}'] = under[n_] / count if count else float('nan')
    return res


def presave_flow(data_root, source='ambient', alpha=1.0, warps=3, iters=64, min_size=8, force=False, report=False, pack=False,
                 device='cuda', disp='gt', tol=0.01):
    """Writes flow.npz into every track directory of data_root that has none (force: into all of them); frames.npz is left untouched,
    each file is replaced atomically.  pack: re-runs packed.pack_dataset.  Returns the number of tracks done, or with report=True -
    which writes nothing - the dict of flow_report (printed as one line).  source 'geometry': the flows come from the `disp` disparities and
    the stored poses (geometry_flows, tol) instead of the images; the report is geometry_report's."""
    data_root = str(data_root)
    geometry = source == 'geometry'
    if report:
        res = geometry_report(data_root, disp, tol, device) if geometry else flow_report(data_root, source, alpha, warps, iters, min_size, device)
        what = f'rigid flow of the {disp} disparities under the stored poses' if geometry else 'flow estimate'
        print(f'{what} against the stored flows over {data_root}: ' + report_text(res, '.4f'))
        return res
    if geometry:
        from .dataset import load_settings
        settings = load_settings(data_root)
    done = 0
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, 'flow.npz')
        if os.path.exists(path) and not force:
            continue
        write_npz(path, geometry_flows(d, disp, settings, tol, device)[0] if geometry else
                  estimate_flows(_frames_of(d, source), alpha, warps, iters, min_size, device))
        done += 1
    if pack:
        packed.pack_dataset(data_root)
    return done


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.presave_flow', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('root')
    ap.add_argument('--source', default='ambient', choices=['ambient', 'im', 'geometry'],
                    help='the array of frames.npz the flows are estimated from; geometry: no image, the flow that --disp and the stored poses imply')
    ap.add_argument('--alpha', type=float, default=1.0, help='weight of the smoothness term')
    ap.add_argument('--warps', type=int, default=3, help='linearisations per pyramid level')
    ap.add_argument('--iters', type=int, default=64, help='Jacobi steps per linearisation')
    ap.add_argument('--min-size', type=int, default=8, help='a pyramid level is added while min(h, w) >= 2 * this')
    ap.add_argument('--disp', default='gt', choices=['gt', 'sgm', 'single_frame', 'multi_frame'], help='--source geometry: which disparities')
    ap.add_argument('--tol', type=float, default=0.01, help='--source geometry: relative depth tolerance of `visible` in --report')
    ap.add_argument('--force', action='store_true', help='also rewrite the flow.npz that exist')
    ap.add_argument('--report', action='store_true', help='compare with the stored flow.npz instead of writing')
    ap.add_argument('--pack', action='store_true', help='also (re)write the packed files (data/packed.py)')
    a = ap.parse_args(argv)
    r = presave_flow(a.root, a.source, a.alpha, a.warps, a.iters, a.min_size, force=a.force, report=a.report, pack=a.pack, disp=a.disp, tol=a.tol)
    if not a.report:
        print(f'{r} tracks done under {a.root}')


if __name__ == '__main__':
    main()
