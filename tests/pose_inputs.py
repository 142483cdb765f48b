"""Inputs and cached restatements shared by the pose tests (tests/test_pose_ref_cpu.py, tests/test_pose_gpu.py)."""
import numpy as np

from tests import pose_ref
from tests.fuse_inputs import punch_holes

# (n, tl, H, W): every pair below min_corr (the failed path); odd, less than one block per row; two tracks and their offsets; all 12
# pairs and many blocks; taller than wide
SHAPES = [(1, 2, 2, 2), (1, 2, 19, 37), (2, 3, 24, 40), (1, 4, 64, 96), (1, 3, 130, 70)]
INPUTS = ['plane', 'bumps', 'noise', 'holes', 'nan_flow', 'no_overlap', 'contam', 'render']
PARAMS = [(6, 1.0, 0.0), (2, 0.5, 1e-3), (12, 2.0, 0.0)]   # (iters, scale, damping)
MIN_CORR = 64
SEEDS = {}   # (shape, kind) -> the seed of synth.make_batch, where it is not 7

_INPUT, _REF = {}, {}


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def has(shape, kind):
    """contam: at 64 x 96 and 130 x 70 only (at 19 x 37 the field of view is +-2.4 degrees and undamped Gauss-Newton on contaminated data
    oscillates: the toy shape's geometry, not behaviour to pin down); render: at 64 x 96 only"""
    if kind == 'contam':
        return shape in (SHAPES[3], SHAPES[4])
    if kind == 'render':
        return shape == SHAPES[3]
    return True


CASES = [(s, k) for s in SHAPES for k in INPUTS if has(s, k)]


def case_id(c):
    return f'{shape_id(c[0])}-{c[1]}'


def pair_truth(R, t):
    """R (n, tl, 3, 3), t (n, tl, 3) -> R_ij = R_j R_i^T (n, tl, tl, 3, 3), t_ij = t_j - R_ij t_i (n, tl, tl, 3), float64"""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    Rp = np.einsum('njab,nicb->nijac', R, R)
    tp = t[:, None, :, :] - np.einsum('nijab,nib->nija', Rp, t)
    return Rp, tp


def stack_flows(get, n, tl, H, W):
    flow = np.zeros((n, tl * tl, 2, H, W), np.float32)
    for i in range(tl):
        for j in range(tl):
            if i != j:
                flow[:, i * tl + j] = get(i, j)
    return flow


def make_input(shape, kind):
    """-> dict: disp (n, tl, H, W), flow (n, tl tl, 2, H, W) float32, K (3, 3) float32, baseline, and the truth R (n, tl, 3, 3), t (n, tl, 3),
    R_pair, t_pair (float64)"""
    key = (shape, kind)
    if key in _INPUT:
        return _INPUT[key]
    from depthinspace_amd import synth
    n, tl, H, W = shape
    if kind == 'render':
        from tests import render_ref, render_scenes
        s = render_scenes.small_settings(H, W)
        disp, flow, Rs, ts = [], [], [], []
        for b in range(n):
            verts, faces, albedo, R, t, blend = render_scenes.small_scene(11 + b, tl)
            r = render_ref.render_ref(verts, faces, albedo, R, t, s.K, s.baseline, blend, s.pattern[..., 0], dtype=np.float64,
                                      ambiguity=False, visibility=False)
            disp.append(r['disp'].reshape(tl, H, W))
            flow.append(r['flow'].reshape(tl * tl, 2, H, W))
            Rs.append(R)
            ts.append(t)
        disp, flow, R, t = np.stack(disp), np.stack(flow), np.stack(Rs), np.stack(ts)
    else:
        s = synth.make_settings(H, W)
        scene = 'bumps' if kind in ('bumps', 'noise', 'contam') else 'plane'
        batch = synth.make_batch(s, n, tl=tl, seed=SEEDS.get(key, 7), scene=scene, motion=0.1, with_primary=False)
        disp = batch['disp0'][:, :, 0].copy()
        flow = stack_flows(lambda i, j: batch[f'flow_{i}{j}'][:, 0], n, tl, H, W)
        R, t = batch['R'], batch['t']
        r = lambda a, b, m: slice(int(a * m), max(int(a * m) + 1, int(b * m)))
        if kind == 'noise':
            rng = np.random.RandomState(5)
            disp += rng.normal(0, 0.05, size=disp.shape).astype(np.float32)
            flow += rng.normal(0, 0.2, size=flow.shape).astype(np.float32)
        elif kind == 'holes':
            punch_holes(disp)
        elif kind == 'nan_flow':
            flow[..., r(0.2, 0.5, H), r(0.3, 0.6, W)] = np.nan
            flow[:, :, 0, r(0.6, 0.8, H), r(0.1, 0.3, W)] = np.inf
            flow[:, :, 1, r(0.6, 0.8, H), r(0.6, 0.9, W)] = -np.inf
        elif kind == 'no_overlap':
            flow += np.float32(2 * W)
        elif kind == 'contam':
            flow[..., :H // 3, :W // 3] += np.float32(3)        # a moving region: the top-left ninth of frame i
            disp[..., r(0.6, 0.65, W)] = 0.0                     # a strip of holes in every frame j
    out = {'disp': disp, 'flow': flow, 'K': s.K, 'baseline': float(s.baseline), 'R': R, 't': t}
    for k in ('disp', 'flow', 'K', 'R', 't'):
        out[k] = np.ascontiguousarray(out[k], dtype=np.float32)
    out['R_pair'], out['t_pair'] = pair_truth(out['R'], out['t'])
    _INPUT[key] = out
    return out


def refs(shape, kind, pi):
    """(float32 restatement, float64 restatement): computed once per case and never changed"""
    key = (shape, kind, pi)
    if key not in _REF:
        a = make_input(shape, kind)
        iters, scale, damping = PARAMS[pi]
        _REF[key] = tuple(pose_ref.track_poses(a['disp'], a['flow'], a['K'], a['baseline'], iters, scale, damping, MIN_CORR, dtype=dt)
                          for dt in (np.float32, np.float64))
    return _REF[key]


def pose_error(r, a):
    """max |R_pair - truth| and max |t_pair - truth| of a restatement or device result r against the truth of the input a"""
    return (float(np.abs(np.asarray(r['R_pair'], dtype=np.float64) - a['R_pair']).max()),
            float(np.abs(np.asarray(r['t_pair'], dtype=np.float64) - a['t_pair']).max()))
