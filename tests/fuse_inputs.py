"""Inputs and cached restatements shared by the track-fusion tests (tests/test_fuse_ref_cpu.py, tests/test_fuse_gpu.py)."""
import numpy as np

from tests import fuse_ref

# (n, tl, H, W): the smallest extent; odd, less than one block per row; per-track counts and offsets; all 12 pairs and many blocks;
# taller than wide
SHAPES = [(1, 2, 2, 2), (1, 2, 19, 37), (2, 3, 24, 40), (1, 4, 64, 96), (1, 3, 130, 70)]
INPUTS = ['plane', 'bumps', 'noise', 'scaled', 'holes', 'render']
PARAMS = [(0.01, 2), (0.002, 1), (0.01, 'tl')]   # (tol, min_views)

_INPUT, _REF = {}, {}


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def params(shape, pi):
    tol, mv = PARAMS[pi]
    return tol, (shape[1] if mv == 'tl' else mv)


def punch_holes(disp):
    """rectangles of 0, NaN, +inf and -1 and a checkerboard patch, at places that scale with the image (in place)"""
    H, W = disp.shape[-2:]
    r = lambda a, b, n: slice(int(a * n), max(int(a * n) + 1, int(b * n)))
    disp[..., r(0.10, 0.25, H), r(0.10, 0.30, W)] = 0.0
    disp[..., r(0.55, 0.70, H), r(0.15, 0.25, W)] = np.nan
    disp[..., r(0.15, 0.30, H), r(0.60, 0.80, W)] = np.inf
    disp[..., r(0.70, 0.85, H), r(0.55, 0.75, W)] = -1.0
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    board = ((ys + xs) % 2 == 0) & (ys >= int(0.40 * H)) & (ys < int(0.55 * H)) & (xs >= int(0.40 * W)) & (xs < int(0.55 * W))
    disp[..., board] = 0.0
    return disp


def make_input(shape, kind):
    """-> dict: disp (n, tl, H, W) float32, R (n, tl, 3, 3), t (n, tl, 3) float32, K (3, 3) float32, baseline, value (n, tl, H, W) float32,
    and for the synthetic kinds `batch` (synth.make_batch)"""
    key = (shape, kind)
    if key in _INPUT:
        return _INPUT[key]
    from depthinspace_amd import synth
    n, tl, H, W = shape
    if kind == 'render':
        from tests import render_ref, render_scenes
        s = render_scenes.small_settings(H, W)
        disp, Rs, ts = [], [], []
        for b in range(n):
            verts, faces, albedo, R, t, blend = render_scenes.small_scene(11 + b, tl)
            r = render_ref.render_ref(verts, faces, albedo, R, t, s.K, s.baseline, blend, s.pattern[..., 0], dtype=np.float64,
                                      ambiguity=False, visibility=False)
            disp.append(r['disp'].reshape(tl, H, W))
            Rs.append(R)
            ts.append(t)
        value = np.random.RandomState(3).uniform(0, 1, shape)
        out = {'disp': np.stack(disp), 'R': np.stack(Rs), 't': np.stack(ts), 'K': s.K, 'baseline': s.baseline, 'value': value}
    else:
        s = synth.make_settings(H, W)
        batch = synth.make_batch(s, n, tl=tl, seed=7, scene='bumps' if kind == 'bumps' else 'plane', motion=0.1, with_primary=False,
                                 with_flow=False)
        disp = batch['disp0'][:, :, 0].copy()
        if kind == 'noise':
            disp *= (1.0 + 0.01 * np.random.RandomState(5).normal(size=shape)).astype(np.float32)
        elif kind == 'scaled':
            disp[:, -1] *= np.float32(1.05)
        elif kind == 'holes':
            punch_holes(disp)
        out = {'disp': disp, 'R': batch['R'], 't': batch['t'], 'K': s.K, 'baseline': s.baseline, 'value': batch['ambient0'][:, :, 0],
               'batch': batch}
    for k in ('disp', 'R', 't', 'K', 'value'):
        out[k] = np.ascontiguousarray(out[k], dtype=np.float32)
    _INPUT[key] = out
    return out


def refs(shape, kind, pi):
    """(float32 restatement, float64 restatement, exempt pixels, exempt pairs): computed once per case and never changed"""
    key = (shape, kind, pi)
    if key not in _REF:
        a = make_input(shape, kind)
        tol, mv = params(shape, pi)
        r32, r64 = (fuse_ref.fuse(a['disp'], a['R'], a['t'], a['K'], a['baseline'], a['value'], tol, mv, dtype=dt)
                    for dt in (np.float32, np.float64))
        ex, ex_pairs = fuse_ref.exempt(r32, r64, tol)
        _REF[key] = (r32, r64, ex, ex_pairs)
    return _REF[key]


def pair_count(shape):
    n, tl, H, W = shape
    return n * tl * (tl - 1) * H * W
