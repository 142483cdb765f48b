"""Semi-global matching presave: the `sgm_disp` array that `--data_type real` training reads (the warm-up term ops.sgm_l1).

For every track directory of a dataset root, the 4 IR frames of frames.npz are matched against the projector pattern of settings.npz
(settings.pattern[..., 0]) with ops.sgm_disparity - 9 x 7 census, 8 paths, uniqueness and left-right checks (include/dis_hip.h, section
"semi-global matching") - and frames.npz is rewritten with sgm_disp (4, 1, H, W) added; invalid pixels hold 0.  The reference takes this
array from the authors' real dataset and has no code that produces it.  Semi-global matching is also the classical baseline of
structured-light depth: --report compares it with the stored ground truth through co/metric.py.

    python -m depthinspace_amd.data.presave_sgm ROOT [--ndisp N] [--p1 P1] [--p2 P2] [--uniq U] [--lr L] [--report] [--pack]
                                                     [--speckle N [--speckle-diff D]] [--fill [GAP] [--fill-dirs K] [--fill-spread S]]
                                                     [--median R] [--refilter]

--speckle N (default 0: off, and then no byte of any file differs) runs the speckle filter ops.speckle_filter on the matcher's output
before it is stored: every 4-connected region of at most N pixels whose neighbouring disparities differ by at most D (--speckle-diff,
default 1.0) is set to 0 (include/dis_hip.h, section "speckle filter").  --refilter applies the same filter to the sgm_disp a track
already stores, in place; the filter is idempotent, so a second run changes nothing.  --report reads what is stored and so shows the
effect.

--fill [GAP] and --median R (both off by default, and then no byte of any file differs) densify what the speckle filter leaves with
ops.disp_densify (include/dis_hip.h, section "disparity densification"); the order is match, speckle, fill, median.  --fill (the bare
flag means a gap of 16) gives an invalid pixel the lower median of the first valid pixels met within GAP steps in the 8 directions when at
least K of them (--fill-dirs, default 6) meet one and these values differ by at most S (--fill-spread, default 2.0): a hole inside one
surface; projector shadows and the columns that can never match stay empty.  --median R (1 or 2) replaces every valid pixel by the
lower median of the valid pixels of its (2 R + 1)^2 window.  When either runs, frames.npz also gets sgm_state (4, 1, H, W) uint8: 0
invalid, 1 matched, 2 filled.  Fill and median are not idempotent, so a track that stores sgm_state is final: --refilter (accepted with
--speckle, --fill or --median) leaves it untouched for every stage and prints how many tracks it skipped.

Known limit: the workers mask the warm-up term with sgm_disp > 30 (the reference's constant).  With the default synthetic geometry
(fx * baseline about 10.7) every rendered disparity is below 30, so the term sees no pixel there; it does with a geometry whose near
disparities exceed 30, as the authors' real sensor has.
"""
import argparse
import os

import numpy as np
import torch

from .dataset import load_settings
from . import packed
from .trackfiles import rewrite_npz

REPORT_THRESHOLDS = (0.1, 0.5, 1, 2, 5)
FLT_MAX = 3.4028234663852886e38


def match_frames(im, pattern, ndisp=64, p1=7, p2=60, uniq=5, lr=1, device='cuda'):
    """im (4, 1, H, W), pattern (H, W) float32 numpy -> sgm_disp (4, 1, H, W) float32 numpy (ops.sgm_disparity on the device)"""
    from .. import ops
    dev = torch.device(device)
    d = ops.sgm_disparity(torch.from_numpy(np.ascontiguousarray(im, dtype=np.float32)).to(dev),
                          torch.from_numpy(np.ascontiguousarray(pattern, dtype=np.float32)).to(dev), ndisp, p1, p2, uniq, lr)
    return d.cpu().numpy()


def filter_speckles(sgm, max_size, max_diff=1.0, device='cuda'):
    """sgm (4, 1, H, W) float32 numpy -> the same with every region of at most max_size pixels set to 0 (ops.speckle_filter on the
    device)"""
    from .. import ops
    d = ops.speckle_filter(torch.from_numpy(np.ascontiguousarray(sgm, dtype=np.float32)).to(torch.device(device)), max_size, max_diff)
    return d.cpu().numpy()


def densify_frames(sgm, max_gap, min_dirs, max_spread, median, device='cuda'):
    """sgm (4, 1, H, W) float32 numpy -> (out, state): the same with the holes inside one surface filled and the median applied, and
    state (4, 1, H, W) uint8 - 0 invalid, 1 valid in sgm, 2 filled (ops.disp_densify on the device)"""
    from .. import ops
    d, state = ops.disp_densify(torch.from_numpy(np.ascontiguousarray(sgm, dtype=np.float32)).to(torch.device(device)), max_gap, min_dirs,
                                max_spread, median, want_state=True)
    return d.cpu().numpy(), state.cpu().numpy().reshape(np.shape(sgm))


def sgm_report(data_root):
    """co/metric.py's DistanceMetric and OutlierFractionMetric of sgm_disp against disp over the pixels where the match is valid
    (sgm_disp != 0) and the surface was seen (disp > 0), over every track of data_root, plus `valid`: the fraction of the seen pixels
    with a valid match.  Needs both arrays in every frames.npz.  Where every frames.npz also stores sgm_state: `filled`, the share of
    the valid pixels that the hole fill wrote (state 2), and `of1_filled`, the share of those more than 1 px off."""
    from ..co import metric
    m = metric.MultipleMetric(metric.DistanceMetric(vec_length=1), metric.OutlierFractionMetric(vec_length=1, thresholds=REPORT_THRESHOLDS))
    seen = valid = filled = filled_off1 = 0
    with_state = True
    for d in packed.track_dirs(data_root):
        with np.load(os.path.join(d, 'frames.npz')) as f:
            if 'sgm_disp' not in f.files or 'disp' not in f.files:
                raise ValueError(f'{d}/frames.npz: --report needs both sgm_disp and disp')
            es, ta = torch.from_numpy(f['sgm_disp']).reshape(-1, 1), torch.from_numpy(f['disp']).reshape(-1, 1)
            state = torch.from_numpy(f['sgm_state']).reshape(-1, 1) if 'sgm_state' in f.files else None
        ma = (es != 0) & (ta > 0)
        with_state = with_state and state is not None
        if with_state:
            fl = ma & (state == 2)
            filled += int(fl.sum())
            filled_off1 += int(((es - ta).abs()[fl] > 1).sum())
        seen += int((ta > 0).sum())
        valid += int(ma.sum())
        m.add(es, ta, ma)
    res = dict(m.get())
    res['valid'] = valid / seen if seen else float('nan')
    if with_state and seen:
        res['filled'] = filled / valid if valid else float('nan')
        res['of1_filled'] = filled_off1 / filled if filled else float('nan')
    return res


def presave_sgm(data_root, ndisp=64, p1=7, p2=60, uniq=5, lr=1, report=False, pack=False, device='cuda', speckle=0, speckle_diff=1.0,
                refilter=False, fill=0, fill_dirs=6, fill_spread=2.0, median=0):
    """Adds sgm_disp (4, 1, H, W) to the frames.npz of every track directory of data_root that has none (incremental; the other arrays
    stay byte-identical; each file is replaced atomically).  speckle > 0: the new array goes through filter_speckles(sgm, speckle,
    speckle_diff) first; refilter: a track that already has sgm_disp gets that array filtered in place (a file the filter does not
    change is not rewritten).  fill > 0 or median > 0: the array then goes through densify_frames(sgm, fill, fill_dirs, fill_spread, median)
    and the state it returns is stored beside it as sgm_state; a track that stores sgm_state is final and refilter skips it (the number
    of such tracks is printed).  pack: re-runs packed.pack_dataset.  Returns the number of tracks written, or with report=True the dict of
    sgm_report (printed as one line)."""
    data_root = str(data_root)
    speckle, speckle_diff = int(speckle), float(speckle_diff)
    if speckle < 0 or not 0 <= speckle_diff < float('inf'):
        raise ValueError('--speckle is a pixel count >= 0 and --speckle-diff a finite disparity difference >= 0')
    fill, fill_dirs, fill_spread, median = int(fill), int(fill_dirs), float(fill_spread), int(median)
    if not (0 <= fill <= 32 and 1 <= fill_dirs <= 8 and 0 <= fill_spread <= FLT_MAX and median in (0, 1, 2)):
        raise ValueError('--fill is a gap of 0 .. 32 pixels, --fill-dirs 1 .. 8, --fill-spread a finite difference >= 0 and --median 0, 1 or 2')
    densify = fill > 0 or median > 0
    if refilter and speckle == 0 and not densify:
        raise ValueError('--refilter needs --speckle N with N > 0, --fill or --median')
    pattern = np.ascontiguousarray(load_settings(data_root).pattern[..., 0], dtype=np.float32)
    done = final = 0
    for d in packed.track_dirs(data_root):
        path = os.path.join(d, 'frames.npz')
        with np.load(path) as f:
            if 'sgm_disp' in f.files and not refilter:
                continue
            if 'sgm_state' in f.files:      # filled or smoothed already: final for every stage
                final += 1
                continue
            stored = f['sgm_disp'] if 'sgm_disp' in f.files else None
            im = f['im'] if stored is None else None
        if stored is None:
            sgm = np.asarray(match_frames(im, pattern, ndisp, p1, p2, uniq, lr, device), dtype=np.float32).reshape(im.shape)
        else:
            sgm = stored
        if speckle > 0:
            sgm = np.asarray(filter_speckles(sgm, speckle, speckle_diff, device), dtype=np.float32).reshape(sgm.shape)
            if not densify and stored is not None and sgm.dtype == stored.dtype and sgm.tobytes() == stored.tobytes():
                continue
        arrays = {'sgm_disp': sgm}
        if densify:
            out, state = densify_frames(sgm, fill, fill_dirs, fill_spread, median, device)
            arrays = {'sgm_disp': np.asarray(out, dtype=np.float32).reshape(sgm.shape),
                      'sgm_state': np.asarray(state, dtype=np.uint8).reshape(sgm.shape)}
        rewrite_npz(path, arrays)
        done += 1
    if final:
        print(f'{final} tracks under {data_root} store sgm_state and were left as they are')
    if pack:
        packed.pack_dataset(data_root)
    if not report:
        return done
    res = sgm_report(data_root)
    print(f'sgm baseline over {data_root} ({done} tracks matched now): valid {res["valid"]:.4f}  ' +
          '  '.join(f'{k} {v:.4f}' for k, v in res.items() if k != 'valid'))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.presave_sgm', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('root')
    ap.add_argument('--ndisp', type=int, default=64, choices=[64, 128, 256], help='disparity candidates 0 .. ndisp - 1')
    ap.add_argument('--p1', type=int, default=7)
    ap.add_argument('--p2', type=int, default=60)
    ap.add_argument('--uniq', type=int, default=5, help='uniqueness margin in per cent')
    ap.add_argument('--lr', type=int, default=1, help='left-right tolerance in pixels')
    ap.add_argument('--report', action='store_true', help='print co/metric.py numbers of sgm_disp against disp')
    ap.add_argument('--pack', action='store_true', help='also (re)write the packed files (data/packed.py)')
    ap.add_argument('--speckle', type=int, default=0, metavar='N',
                    help='set regions of at most N pixels of similar disparity to 0 before storing (0: off)')
    ap.add_argument('--speckle-diff', type=float, default=1.0, metavar='D', help='largest disparity step inside a region')
    ap.add_argument('--fill', type=int, nargs='?', const=16, default=0, metavar='GAP',
                    help='fill holes inside one surface from the first valid pixels within GAP steps in 8 directions (0: off; bare: 16)')
    ap.add_argument('--fill-dirs', type=int, default=6, metavar='K', help='directions that must meet a valid pixel (1 .. 8)')
    ap.add_argument('--fill-spread', type=float, default=2.0, metavar='S', help='largest difference among the values met')
    ap.add_argument('--median', type=int, default=0, choices=[0, 1, 2], metavar='R',
                    help='lower median over the valid pixels of a (2 R + 1)^2 window (0: off)')
    ap.add_argument('--refilter', action='store_true',
                    help='also filter the sgm_disp that tracks already store (needs --speckle, --fill or --median)')
    a = ap.parse_args(argv)
    r = presave_sgm(a.root, a.ndisp, a.p1, a.p2, a.uniq, a.lr, report=a.report, pack=a.pack, speckle=a.speckle,
                    speckle_diff=a.speckle_diff, refilter=a.refilter, fill=a.fill, fill_dirs=a.fill_dirs, fill_spread=a.fill_spread,
                    median=a.median)
    if not a.report:
        print(f'{r} tracks {"written" if a.refilter else "matched"} under {a.root}')


if __name__ == '__main__':
    main()
