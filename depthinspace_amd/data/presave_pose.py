"""Pose presave: the camera poses `R` and `t` of frames.npz - which the geometric loss of both workers, FuseNet and data/fuse.py read - for
tracks that arrive without them.

Rendered and synthetic tracks carry exact poses; a captured track has images only.  Once it has a disparity per frame (sgm_disp from
data/presave_sgm.py, or a network's from data/presave_disp.py) and a flow per ordered frame pair (data/presave_flow.py), the two are
dense 3D - 3D correspondences.  For every track directory of a dataset root the chosen disparities and flow.npz go with the K and
baseline of settings.npz through ops.track_poses - Gauss-Newton per ordered frame pair on the residual in (u, v, disparity), with a
redescending weight (include/dis_hip.h, section "track poses") - up to four tracks per call.  Frame 0 becomes the world (R_0 = I,
t_0 = 0); frame j takes the pair (0, j), or the inverse of the pair (j, 0) where that one failed.  R (tl, 3, 3) and t (tl, 3) are added
to frames.npz through a temporary file; its other arrays stay byte-identical and nothing else is touched.  A track with a frame both of
whose pairs failed is listed as failed and left as it is.

    python -m depthinspace_amd.data.presave_pose ROOT [--disp gt|sgm|single_frame|multi_frame] [--iters N] [--scale S] [--damping D]
                                                      [--min-corr N] [--force] [--report] [--pack] [--joint] [--joint-iters N]
                                                      [--pairwise flow|disp]
                                                      [--model] [--model-rounds N] [--model-iters N] [--res N | --voxel V]
                                                      [--trunc VOXELS] [--min-weight N] [--tol T] [--min-views N]

A track that already stores R and t is skipped unless --force is given: rendered tracks keep their exact poses.  --report also
estimates the tracks that are skipped and prints one line over the dataset: the pairs that are ok / failed, the mean share of the
pixels a pair uses, its mean weight and weighted rms residual in pixels, and the cycle error - the rotation angle of R_ji R_ij and
|t_ji + R_ji t_ij| over the median depth of the track, averaged over the unordered pairs: a quality figure that needs no ground truth.
Where a track stored poses before the run, the rotation angle and the translation error (over the median depth) of the estimated
relative poses against the stored ones are added.

--pairwise disp takes the pairwise stage from the disparity maps alone, ops.disp_align_poses (dis_disp_align_poses; include/dis_hip.h,
section "disparity alignment"): direct coarse-to-fine alignment of frame i's disparity map onto frame j's, from the identity, with no
flow - no flow.npz is needed, and data/presave_flow.py --source geometry can then write one from the poses.  It is what to use where
the images carry no texture for an image-based flow (flat-shaded surfaces: there the flow-based poses are wrong by the size of the
motion itself), and what gives --model a start inside its truncation band.  It runs at its own defaults (levels, schedule, a robust
scale of 0.3 px of disparity); --iters and --scale belong to the flow-based stage, --damping and --min-corr to both.  Its limits: the scene must be static;
the disparity noise must be small against the disparity (at 10 % it breaks down); a planar fronto-parallel scene leaves three of the six
directions open and the pair fails at a zero pivot; holes take no part.  The outputs, the composition, --report, --force, --pack and
--model are those of the flow-based stage; --joint still reads flow.npz and says so where there is none.

Without --joint this is pairwise and nothing more: the pairs are independent, and only the pairs with frame 0 set the stored poses.
--joint adds a second stage, ops.refine_track_poses (dis_refine_track_poses): one pose per frame, frame 0 fixed, --joint-iters
Gauss-Newton steps on the residuals of all ordered pairs that the pairwise stage reports as ok at once - the same per-pixel terms, one
6 (tl - 1) system per track - so that one bad pair with frame 0 is corrected by the pairs among the other frames, and the frames 1 ..
tl - 1 are fitted to each other.  It starts from the pairwise result; a frame both of whose pairs with frame 0 failed is reached
through the other ok pairs (chain_track), and such a track is no longer listed as failed.  A track whose joint system is singular is
written with its composed pairwise poses and counted (`joint_failed`); --report adds the joint rms residual over the contributing
pairs, their share of the ordered pairs, and against stored poses the errors of the joint poses (`joint_gt_rot`, `joint_gt_trans`,
over all ordered pairs) next to the pairwise ones.  Still not done: the intrinsics are taken as given, there is no loop closure
across tracks, no step control beyond the damping term, and a track has at most four frames.

--model adds a last stage before the poses are written, after the pairwise estimate and, if given, --joint: frame-to-model refinement,
the tracking step of KinectFusion (ops.tsdf_align_poses / dis_tsdf_align_poses).  The poses so far place one lattice around the track as
data/mesh.py does (--res or --voxel, --trunc, --tol, --min-views); then, for --model-rounds rounds and each frame but the first, the
other frames are integrated into that lattice at their current poses and the frame is aligned to the volume by --model-iters
Gauss-Newton steps on the signed distance of its back-projected pixels to the surface - leave-one-out, because a model that already
holds the frame at its old pose would keep it there.  A frame whose alignment fails keeps its pose and is counted.  It reads no flow, so
it measures the poses against the geometry they produce - which the flow-based stages cannot; it needs disparities good enough to fuse:
run it with --disp single_frame or multi_frame and --force once the networks exist.  --report adds `model_resid_before` and
`model_resid_after` (the weighted rms distance of a frame to the model in voxels, averaged over the aligned frames: the opening pass of
round 1 and the closing pass of the last round), `model_used` (the share of the valid pixels used), `model_failed`, and against stored
poses `model_gt_rot`, `model_gt_trans` next to the pairwise and joint ones.  Its limits: the capture range is about the truncation band
(--trunc voxels: the start must already be that close); its accuracy is bounded by the volume, a fraction of a voxel, so poses that
are already better than that - exact disparities with good flows - are made worse, not better (profiles/tsdf_align_rate.md has the
figures); on a planar scene the residual falls while the pose slides along the
directions the surface does not constrain; the intrinsics are not refined, and there is no loop closure across tracks.  Without --model
nothing changes, the bytes written included.
"""
import argparse
import os

import numpy as np
import torch

from . import packed
from .dataset import load_settings
from .trackfiles import SOURCES, load_disp, report_text, rewrite_npz

BATCH = 4


def load_flow(d, tl):
    """flow.npz -> (tl tl, 2, H, W) float32 in the layout of ops.dense_flow, zeros on the diagonal"""
    path = os.path.join(d, 'flow.npz')
    if not os.path.exists(path):
        raise ValueError(f'{path} is missing (data/presave_flow.py writes it)')
    with np.load(path) as f:
        pairs = {(i, j): np.asarray(f[f'flow_{i}{j}'], dtype=np.float32) for i in range(tl) for j in range(tl) if i != j}
    h, w = pairs[(0, 1)].shape[-2:]
    flow = np.zeros((tl * tl, 2, h, w), np.float32)
    for (i, j), a in pairs.items():
        flow[i * tl + j] = a.reshape(2, h, w)
    return flow


def stored_poses(d):
    """(R, t) of frames.npz, or None where it has none"""
    with np.load(os.path.join(d, 'frames.npz')) as f:
        if 'R' in f.files and 't' in f.files:
            return f['R'], f['t']
    return None


def compose_track(R_pair, t_pair, ok):
    """R_pair (tl, tl, 3, 3), t_pair (tl, tl, 3) (X_j = R_ij X_i + t_ij), ok (tl, tl) bool -> R (tl, 3, 3), t (tl, 3) float32 with frame 0
    the world: frame j takes the pair (0, j), or the inverse of the pair (j, 0) where that one failed; None if both failed for a frame"""
    tl = R_pair.shape[0]
    R, t = np.zeros((tl, 3, 3), np.float64), np.zeros((tl, 3), np.float64)
    R[0] = np.eye(3)
    for j in range(1, tl):
        if ok[0, j]:
            R[j], t[j] = R_pair[0, j], t_pair[0, j]
        elif ok[j, 0]:
            Rj0 = np.asarray(R_pair[j, 0], dtype=np.float64)
            R[j], t[j] = Rj0.T, -Rj0.T @ np.asarray(t_pair[j, 0], dtype=np.float64)
        else:
            return None
    return R.astype(np.float32), t.astype(np.float32)


def chain_track(R_pair, t_pair, ok):
    """compose_track for the start of the joint refinement: a frame both of whose pairs with frame 0 failed is reached through the ok
    pairs instead.  A breadth-first walk from frame 0: the frames reached are visited in the order they were reached, and each one
    gives its pose to the frames not reached yet, in index order, through the pair (a, b) or the inverse of the pair (b, a) where
    that one failed.  A frame next to frame 0 gets the values of compose_track.  None if a frame cannot be reached at all."""
    tl = R_pair.shape[0]
    R, t = np.zeros((tl, 3, 3), np.float64), np.zeros((tl, 3), np.float64)
    R[0] = np.eye(3)
    reached, queue = {0}, [0]
    while queue:
        a = queue.pop(0)
        for b in range(tl):
            if b in reached or not (ok[a, b] or ok[b, a]):
                continue
            if ok[a, b]:
                Rab, tab = np.asarray(R_pair[a, b], dtype=np.float64), np.asarray(t_pair[a, b], dtype=np.float64)
            else:
                Rba = np.asarray(R_pair[b, a], dtype=np.float64)
                Rab, tab = Rba.T, -Rba.T @ np.asarray(t_pair[b, a], dtype=np.float64)
            R[b], t[b] = Rab @ R[a], Rab @ t[a] + tab
            reached.add(b)
            queue.append(b)
    if len(reached) < tl:
        return None
    return R.astype(np.float32), t.astype(np.float32)


def relative_poses(R, t):
    """R (tl, 3, 3), t (tl, 3) -> R_ij = R_j R_i^T (tl, tl, 3, 3), t_ij = t_j - R_ij t_i (tl, tl, 3), float64"""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    Rp = np.einsum('jab,icb->ijac', R, R)
    return Rp, t[None, :, :] - np.einsum('ijab,ib->ija', Rp, t)


def rotation_angle(R):
    """the angle of the rotation(s) R (..., 3, 3) in radians: atan2 of the length of the skew part and (trace - 1) / 2, which stays
    accurate at small angles where the arc cosine of the trace does not"""
    R = np.asarray(R, dtype=np.float64)
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    return np.arctan2(np.linalg.norm(s, axis=-1), 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0))


def median_depth(disp, fb):
    """the median of fb / disp over the valid pixels of a track (nan without any)"""
    d = np.asarray(disp, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(d) & (d > 0)
    return float(np.median(fb / d[ok])) if ok.any() else float('nan')


def report_terms(R_pair, t_pair, stats, pixels, depth, stored=None):
    """the sums one track adds to the report.  R_pair (tl, tl, 3, 3), t_pair (tl, tl, 3), stats (tl, tl, 4) of ops.track_poses, pixels =
    H W, depth = the track's median depth, stored = (R, t) or None -> dict: ok, failed (ordered pairs); share, weight, resid (sums over
    the ok pairs of n / pixels, the mean weight, the rms residual); cycles, cycle_rot, cycle_trans (unordered pairs both of whose
    directions are ok, and the sums over them); and with stored poses gt_pairs, gt_rot, gt_trans (sums over the ok pairs)"""
    R_pair, t_pair, stats = (np.asarray(a, dtype=np.float64) for a in (R_pair, t_pair, stats))
    tl = R_pair.shape[0]
    off = ~np.eye(tl, dtype=bool)
    ok = (stats[..., 3] != 0) & off
    r = {'ok': int(ok.sum()), 'failed': int((off & ~ok).sum()), 'share': float((stats[..., 0][ok] / pixels).sum()),
         'weight': float(stats[..., 1][ok].sum()), 'resid': float(stats[..., 2][ok].sum()), 'cycles': 0, 'cycle_rot': 0.0, 'cycle_trans': 0.0}
    for i in range(tl):
        for j in range(i + 1, tl):
            if ok[i, j] and ok[j, i]:
                r['cycles'] += 1
                r['cycle_rot'] += float(rotation_angle(R_pair[j, i] @ R_pair[i, j]))
                r['cycle_trans'] += float(np.linalg.norm(t_pair[j, i] + R_pair[j, i] @ t_pair[i, j]) / depth)
    if stored is not None:
        Rs, ts = relative_poses(*stored)
        r['gt_pairs'] = int(ok.sum())
        r['gt_rot'] = float(rotation_angle(R_pair[ok] @ np.swapaxes(Rs[ok], -1, -2)).sum())
        r['gt_trans'] = float((np.linalg.norm(t_pair[ok] - ts[ok], axis=-1) / depth).sum())
    return r


def report_line(acc):
    """the sums of report_terms added over the tracks -> the dict that is printed"""
    div = lambda a, b: a / b if b else float('nan')
    res = {'ok': acc['ok'], 'failed': acc['failed'], 'share': div(acc['share'], acc['ok']), 'weight': div(acc['weight'], acc['ok']),
           'resid': div(acc['resid'], acc['ok']), 'cycle_rot': div(acc['cycle_rot'], acc['cycles']),
           'cycle_trans': div(acc['cycle_trans'], acc['cycles'])}
    if acc.get('gt_pairs'):
        res['gt_rot'] = acc['gt_rot'] / acc['gt_pairs']
        res['gt_trans'] = acc['gt_trans'] / acc['gt_pairs']
    return res


def estimate_pairs(disps, flows, settings, iters=6, scale=1.0, damping=0.0, min_corr=64, device='cuda'):
    """lists of (tl, H, W) disparities and (tl tl, 2, H, W) flows of tracks of one length, float32 numpy -> R_pair (n, tl, tl, 3, 3),
    t_pair (n, tl, tl, 3), stats (n, tl, tl, 4) float32 numpy (one call of ops.track_poses)"""
    from .. import ops
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.stack(a), dtype=np.float32)).to(dev)
    r = ops.track_poses(up(disps), up(flows), np.asarray(settings.K, dtype=np.float32), settings.baseline, iters=iters, scale=scale,
                        damping=damping, min_corr=min_corr)
    return tuple(r[k].cpu().numpy() for k in ('R_pair', 't_pair', 'stats'))


def align_pairs(disps, settings, damping=0.0, min_corr=64, device='cuda'):
    """estimate_pairs without flows: a list of (tl, H, W) disparities of tracks of one length -> R_pair, t_pair, stats float32 numpy (one
    call of ops.disp_align_poses at its default levels and schedule)"""
    from .. import ops
    d = torch.from_numpy(np.ascontiguousarray(np.stack(disps), dtype=np.float32)).to(torch.device(device))
    r = ops.disp_align_poses(d, np.asarray(settings.K, dtype=np.float32), settings.baseline, damping=damping, min_corr=min_corr)
    return tuple(r[k].cpu().numpy() for k in ('R_pair', 't_pair', 'stats'))


def refine_tracks(disps, flows, settings, R_init, t_init, use, iters=6, scale=1.0, damping=0.0, min_corr=64, device='cuda'):
    """the lists of estimate_pairs with R_init (n, tl, 3, 3), t_init (n, tl, 3) float32 and use (n, tl, tl) bool -> R (n, tl, 3, 3), t (n, tl, 3),
    pair_stats (n, tl, tl, 4), track_stats (n, 4) float32 numpy (one call of ops.refine_track_poses)"""
    from .. import ops
    dev = torch.device(device)
    up = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    r = ops.refine_track_poses(up(np.stack(disps)), up(np.stack(flows)), np.asarray(settings.K, dtype=np.float32), settings.baseline,
                               up(R_init), up(t_init), up(use, np.uint8), iters=iters, scale=scale, damping=damping, min_corr=min_corr)
    return tuple(r[k].cpu().numpy() for k in ('R', 't', 'pair_stats', 'track_stats'))


def joint_terms(R, t, track_stats, depth, stored=None):
    """the sums one jointly refined track adds to the report.  R (tl, 3, 3), t (tl, 3), track_stats (4) of ops.refine_track_poses -> dict:
    joint_tracks (1), joint_failed (status 0: nothing else is added), joint_resid (the rms residual over the contributing pairs),
    joint_share (their share of the ordered pairs); with stored poses joint_gt_pairs (all ordered pairs), joint_gt_rot, joint_gt_trans"""
    tl = len(R)
    if track_stats[3] == 0:
        return {'joint_tracks': 1, 'joint_failed': 1}
    r = {'joint_tracks': 1, 'joint_failed': 0, 'joint_resid': float(track_stats[2]), 'joint_share': float(track_stats[0]) / (tl * (tl - 1))}
    if stored is not None:
        off = ~np.eye(tl, dtype=bool)
        (Rj, tj), (Rs, ts) = relative_poses(R, t), relative_poses(*stored)
        r['joint_gt_pairs'] = int(off.sum())
        r['joint_gt_rot'] = float(rotation_angle(Rj[off] @ np.swapaxes(Rs[off], -1, -2)).sum())
        r['joint_gt_trans'] = float((np.linalg.norm(tj[off] - ts[off], axis=-1) / depth).sum())
    return r


def joint_line(acc):
    """the sums of joint_terms added over the tracks -> what the joint stage adds to the dict that is printed"""
    div = lambda a, b: a / b if b else float('nan')
    good = acc['joint_tracks'] - acc['joint_failed']
    res = {'joint_resid': div(acc.get('joint_resid', 0.0), good), 'joint_share': div(acc.get('joint_share', 0.0), good)}
    if acc.get('joint_gt_pairs'):
        res['joint_gt_rot'] = acc['joint_gt_rot'] / acc['joint_gt_pairs']
        res['joint_gt_trans'] = acc['joint_gt_trans'] / acc['joint_gt_pairs']
    return res


def model_loop(R, t, integrate, align, rounds=2):
    """the leave-one-out loop of the model stage, Gauss-Seidel: for each round and each frame f = 1 .. tl - 1, vol = integrate(others, R, t)
    - the frames `others` (all but f) at their current poses - and align(f, vol, R[f], t[f]) -> (R_f, t_f, stats (8) of
    ops.tsdf_align_poses), taken where its status is 1.  Aligning a frame to a model that already holds it at its old pose would keep
    it there; frame 0 stays the world.  R (tl, 3, 3), t (tl, 3) float32 -> R, t (copies), first, last: the stats (tl, 8) of every frame's
    alignment in the first and in the last round (row 0: zeros)"""
    R, t = np.array(R, dtype=np.float32), np.array(t, dtype=np.float32)
    tl = len(R)
    first, last = np.zeros((tl, 8), np.float32), np.zeros((tl, 8), np.float32)
    for r in range(int(rounds)):
        for f in range(1, tl):
            vol = integrate([k for k in range(tl) if k != f], R, t)
            Rf, tf, st = align(f, vol, R[f], t[f])
            if r == 0:
                first[f] = st
            last[f] = st
            if st[3] == 1:
                R[f], t[f] = Rf, tf
    return R, t, first, last


def model_refine_track(disp, R, t, value, settings, rounds=2, iters=6, res=256, voxel=None, trunc_voxels=3.0, min_weight=1, tol=0.01,
                       min_views=2, scale=None, damping=0.0, min_corr=64, device='cuda'):
    """one track, float32 numpy in: frame-to-model refinement of its poses (ops.tsdf_align_poses) against its own volume.  The lattice
    is placed once, from the incoming poses, as data/mesh.py places it (mesh.place_track); then model_loop, with the other frames
    integrated into that lattice by mesh.integrate_placed and `iters` steps per alignment.  -> dict R (tl, 3, 3), t (tl, 3) float32
    numpy, first, last (tl, 8: see model_loop), voxel, trunc, grid - or None where the volume cannot be placed"""
    from .. import ops
    from . import mesh
    disp = np.ascontiguousarray(disp, dtype=np.float32)
    disp = disp.reshape(disp.shape[0], disp.shape[-2], disp.shape[-1])
    place = mesh.place_track(disp, R, t, value, settings, res, voxel, trunc_voxels, tol, min_views, device)
    if place is None:
        return None
    origin, vx, trunc, grid = place
    dev = torch.device(device)
    K = np.asarray(settings.K, dtype=np.float32)
    d_disp = torch.from_numpy(disp).to(dev)
    ws = torch.empty(ops.lib.fn('dis_tsdf_align_workspace')(1, disp.shape[1], disp.shape[2]), dtype=torch.uint8, device=dev)

    def integrate(others, Rc, tc):
        return mesh.integrate_placed(disp[others], Rc[others], tc[others], None if value is None else np.asarray(value)[others], settings,
                                     place, device)

    def align(f, vol, Rf, tf):
        r = ops.tsdf_align_poses(vol['tsdf'], vol['weight'], origin, vx, trunc, d_disp[f:f + 1], K, settings.baseline,
                                 torch.from_numpy(Rf[None].copy()).to(dev), torch.from_numpy(tf[None].copy()).to(dev), iters=iters, scale=scale,
                                 damping=damping, min_corr=min_corr, min_weight=min_weight, workspace=ws)
        return r['R'][0].cpu().numpy(), r['t'][0].cpu().numpy(), r['stats'][0].cpu().numpy()

    Rn, tn, first, last = model_loop(R, t, integrate, align, rounds)
    return dict(R=Rn, t=tn, first=first, last=last, voxel=vx, trunc=trunc, grid=grid)


def model_terms(res, depth, stored=None):
    """the sums one track adds to the report for the model stage.  res: the dict of model_refine_track -> dict: model_frames (the frames
    aligned in the first and in the last round, over which the next three are summed), model_resid_before, model_resid_after (the
    weighted rms distance to the model in voxels: the opening pass of round 1, the closing pass of the last round), model_used (the
    share of the valid pixels that the closing pass uses), model_failed (frames whose last alignment failed); with stored poses
    model_gt_pairs (all ordered pairs), model_gt_rot, model_gt_trans"""
    first, last = res['first'][1:], res['last'][1:]
    ok = (first[:, 3] == 1) & (last[:, 3] == 1)
    r = {'model_frames': int(ok.sum()), 'model_failed': int((last[:, 3] != 1).sum()),
         'model_resid_before': float((first[ok, 6] / res['voxel']).sum()), 'model_resid_after': float((last[ok, 2] / res['voxel']).sum()),
         'model_used': float((last[ok, 0] / np.maximum(last[ok, 7], 1)).sum())}
    if stored is not None:
        tl = len(res['R'])
        off = ~np.eye(tl, dtype=bool)
        (Rm, tm), (Rs, ts) = relative_poses(res['R'], res['t']), relative_poses(*stored)
        r['model_gt_pairs'] = int(off.sum())
        r['model_gt_rot'] = float(rotation_angle(Rm[off] @ np.swapaxes(Rs[off], -1, -2)).sum())
        r['model_gt_trans'] = float((np.linalg.norm(tm[off] - ts[off], axis=-1) / depth).sum())
    return r


def model_line(acc):
    """the sums of model_terms added over the tracks -> what the model stage adds to the dict that is printed"""
    div = lambda a, b: a / b if b else float('nan')
    n = acc.get('model_frames', 0)
    res = {'model_resid_before': div(acc.get('model_resid_before', 0.0), n), 'model_resid_after': div(acc.get('model_resid_after', 0.0), n),
           'model_used': div(acc.get('model_used', 0.0), n), 'model_failed': acc.get('model_failed', 0)}
    if acc.get('model_gt_pairs'):
        res['model_gt_rot'] = acc['model_gt_rot'] / acc['model_gt_pairs']
        res['model_gt_trans'] = acc['model_gt_trans'] / acc['model_gt_pairs']
    return res


def presave_pose(data_root, source='sgm', iters=6, scale=1.0, damping=0.0, min_corr=64, force=False, report=False, pack=False,
                 device='cuda', joint=False, joint_iters=6, model=False, model_rounds=2, model_iters=6, res=256, voxel=None, trunc_voxels=3.0,
                 min_weight=1, tol=0.01, min_views=2, pairwise='flow'):
    """Adds R (tl, 3, 3) and t (tl, 3) to the frames.npz of every track directory of data_root that has none (force: of all of them),
    each through a temporary file; the other arrays stay byte-identical.  pack: re-runs packed.pack_dataset.  Returns the number of
    tracks written, or with report=True - which also estimates the tracks it does not write - the dict of report_line with `tracks`,
    `written` and `failed_tracks` added (printed as one line).  The tracks that failed are printed by name.  joint: the pairwise result
    is refined by ops.refine_track_poses (joint_iters steps) before it is written - see the module's docstring; the report then also
    carries the keys of joint_line and `joint_failed`, the tracks written with their pairwise poses.  model: the poses - pairwise, or
    joint - are then refined against the track's own volume by model_refine_track (model_rounds leave-one-out rounds of model_iters steps;
    res, voxel, trunc_voxels, min_weight, tol, min_views as in data/mesh.py) before they are written; a track whose volume cannot be
    placed keeps the poses it came with; the report then also carries the keys of model_line.  pairwise 'disp': the pairwise stage is
    align_pairs and reads no flow.npz; joint still does."""
    if pairwise not in ('flow', 'disp'):
        raise ValueError(f'pairwise must be flow or disp, not {pairwise!r}')
    data_root = str(data_root)
    settings = load_settings(data_root)
    K = np.asarray(settings.K, dtype=np.float64)
    fb = float(K[0, 0]) * float(settings.baseline)
    todo = []
    for d in packed.track_dirs(data_root):
        stored = stored_poses(d)
        write = force or stored is None
        if write or report:
            todo.append((d, write, stored))
    done, failed, joint_failed, acc, k = 0, [], [], {}, 0
    while k < len(todo):
        disps, flows = [], []
        while k < len(todo) and len(disps) < BATCH:       # up to four tracks of one length per call
            disp = load_disp(todo[k][0], source)
            if disps and disp.shape != disps[0].shape:
                break
            disps.append(disp)
            if pairwise == 'flow' or joint:
                if joint and not os.path.exists(os.path.join(todo[k][0], 'flow.npz')):
                    raise ValueError(f'{todo[k][0]}: --joint reads flow.npz and there is none (data/presave_flow.py writes it; with '
                                     f'--pairwise disp run without --joint first, then presave_flow --source geometry)')
                flows.append(load_flow(todo[k][0], disp.shape[0]))
            k += 1
        if pairwise == 'disp':
            Rp, tp, st = align_pairs(disps, settings, damping, min_corr, device)
        else:
            Rp, tp, st = estimate_pairs(disps, flows, settings, iters, scale, damping, min_corr, device)
        ok = st[..., 3] != 0
        if joint:
            # the start: the pairwise result chained from frame 0; a track that no chain covers takes no part (no pair is used: it fails)
            starts = [chain_track(Rp[b], tp[b], ok[b]) for b in range(len(disps))]
            tl = disps[0].shape[0]
            R0 = np.stack([np.broadcast_to(np.eye(3, dtype=np.float32), (tl, 3, 3)) if s_ is None else s_[0] for s_ in starts])
            t0 = np.stack([np.zeros((tl, 3), np.float32) if s_ is None else s_[1] for s_ in starts])
            use = np.stack([ok[b] & (starts[b] is not None) for b in range(len(disps))])
            Rj, tj, _, jst = refine_tracks(disps, flows, settings, R0, t0, use, joint_iters, scale, damping, min_corr, device)
        for b, (d, write, stored) in enumerate(todo[k - len(disps):k]):
            if report:
                depth = median_depth(disps[b], fb)
                terms = report_terms(Rp[b], tp[b], st[b], disps[b].shape[-2] * disps[b].shape[-1], depth, stored)
                if joint and starts[b] is not None:
                    terms.update(joint_terms(Rj[b], tj[b], jst[b], depth, stored))
                for key, v in terms.items():
                    acc[key] = acc.get(key, 0) + v
            if not (write or (model and report)):
                continue
            if joint:
                poses = starts[b]
                if poses is not None and jst[b, 3] != 0:
                    poses = (Rj[b], tj[b])
                elif poses is not None and write:
                    joint_failed.append(d)
            else:
                poses = compose_track(Rp[b], tp[b], ok[b])
            if model and poses is not None:
                mres = model_refine_track(disps[b], poses[0], poses[1], None, settings, model_rounds, model_iters, res, voxel, trunc_voxels,
                                          min_weight, tol, min_views, device=device)
                if mres is not None:
                    poses = (mres['R'], mres['t'])
                    if report:
                        for key, v in model_terms(mres, depth, stored).items():
                            acc[key] = acc.get(key, 0) + v
            if not write:
                continue
            if poses is None:
                failed.append(d)
                continue
            rewrite_npz(os.path.join(d, 'frames.npz'), {'R': poses[0], 't': poses[1]})
            done += 1
    if failed:
        why = 'a frame that no chain of estimated pairs reaches from frame 0' if joint else 'a frame without an estimated pair with frame 0'
        print(f'{len(failed)} tracks failed ({why}) and were left as they are: ' + ', '.join(os.path.basename(d) for d in failed))
    if joint_failed:
        print(f'{len(joint_failed)} tracks were written with their pairwise poses (the joint system was singular): '
              + ', '.join(os.path.basename(d) for d in joint_failed))
    if pack:
        packed.pack_dataset(data_root)
    if not report:
        return done
    out = report_line(acc) if acc else {}
    if acc.get('joint_tracks'):
        out.update(joint_line(acc))
    out.update(tracks=len(todo), written=done, failed_tracks=len(failed))
    if joint:
        out.update(joint_failed=len(joint_failed))
    if model:
        out.update(model_line(acc))
    stage = 'aligned disparity maps' if pairwise == 'disp' else f'iters {iters}, scale {scale:g}'
    print(f'poses from the {source} disparities over {data_root} ({stage}, damping {damping:g}'
          + (f', joint iters {joint_iters}' if joint else '') + (f', model rounds {model_rounds} iters {model_iters}' if model else '') + '): ' + report_text(out, '.6g'))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.presave_pose', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('root')
    ap.add_argument('--disp', default='sgm', choices=SOURCES, help='which disparities the poses are estimated from')
    ap.add_argument('--iters', type=int, default=6, help='Gauss-Newton steps per frame pair (1 .. 64)')
    ap.add_argument('--scale', type=float, default=1.0, help='scale of the redescending weight, in pixels')
    ap.add_argument('--damping', type=float, default=0.0, help='this times diag(H) is added to the normal matrix')
    ap.add_argument('--min-corr', type=int, default=64, help='a pair with fewer usable pixels fails')
    ap.add_argument('--force', action='store_true', help='also rewrite the poses that are stored')
    ap.add_argument('--report', action='store_true', help='also print the quality figures over the dataset')
    ap.add_argument('--pack', action='store_true', help='also (re)write the packed files (data/packed.py)')
    ap.add_argument('--joint', action='store_true', help='refine the poses of a track jointly over all its ok pairs before they are written')
    ap.add_argument('--joint-iters', type=int, default=6, help='Gauss-Newton steps of the joint refinement (1 .. 64)')
    ap.add_argument('--model', action='store_true', help="refine the poses against the track's own TSDF volume before they are written")
    ap.add_argument('--model-rounds', type=int, default=2, help='leave-one-out rounds over the frames of a track')
    ap.add_argument('--model-iters', type=int, default=6, help='Gauss-Newton steps of one alignment (1 .. 64)')
    size = ap.add_mutually_exclusive_group()
    size.add_argument('--res', type=int, default=256, help='--model: lattice points along the longest side of the padded box')
    size.add_argument('--voxel', type=float, default=None, help='--model: the lattice spacing, instead of --res')
    ap.add_argument('--trunc', type=float, default=3.0, help='--model: the truncation distance in voxels')
    ap.add_argument('--min-weight', type=int, default=1, help='--model: frames that must observe each of the eight lattice points of a cell')
    ap.add_argument('--tol', type=float, default=0.01, help='--model: relative depth tolerance of the cross-view check that places the volume')
    ap.add_argument('--min-views', type=int, default=2, help='--model: agreeing frames a point needs to count for the placement')
    ap.add_argument('--pairwise', default='flow', choices=['flow', 'disp'],
                    help='the pairwise stage: disparities and flow.npz (flow), or the disparity maps alone (disp: no flow.npz is needed)')
    a = ap.parse_args(argv)
    if a.voxel is not None and not a.voxel > 0:
        ap.error('--voxel must be positive')
    if not a.trunc > 0:
        ap.error('--trunc must be positive')
    if a.model_rounds < 1:
        ap.error('--model-rounds must be at least 1')
    r = presave_pose(a.root, a.disp, a.iters, a.scale, a.damping, a.min_corr, force=a.force, report=a.report, pack=a.pack, joint=a.joint,
                     joint_iters=a.joint_iters, model=a.model, model_rounds=a.model_rounds, model_iters=a.model_iters, res=a.res, voxel=a.voxel,
                     trunc_voxels=a.trunc, min_weight=a.min_weight, tol=a.tol, min_views=a.min_views, pairwise=a.pairwise)
    print(f'{r["written"] if a.report else r} tracks written under {a.root}')


if __name__ == '__main__':
    main()
