"""Inputs and cached restatements shared by the volumetric-fusion tests (tests/test_tsdf_ref_cpu.py, tests/test_tsdf_gpu.py)."""
import numpy as np

from tests import fuse_inputs, tsdf_ref

KINDS = ['plane', 'bumps', 'noise', 'holes', 'render']
# image shapes (tl, H, W): track 0 of these fuse_inputs shapes
SHAPES = {(2, 19, 37): (1, 2, 19, 37), (3, 24, 40): (2, 3, 24, 40), (4, 64, 96): (1, 4, 64, 96)}
# (nx, ny, nz): a single cell; odd, less than one block; rows that are no multiple of 64; several blocks; 1056 blocks of 256 lattice
# points, more than one pass of the 1024-wide scan
GRIDS = [(2, 2, 2), (7, 3, 5), (33, 17, 20), (40, 40, 48), (66, 64, 64)]

_INPUT, _VOLUME, _REF = {}, {}, {}


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def make_input(shape, kind):
    """-> dict: disp (tl, H, W), R (tl, 3, 3), t (tl, 3), K (3, 3), value (tl, H, W) float32, baseline"""
    key = (shape, kind)
    if key not in _INPUT:
        a = fuse_inputs.make_input(SHAPES[shape], kind)
        _INPUT[key] = {'disp': a['disp'][0], 'R': a['R'][0], 't': a['t'][0], 'K': a['K'], 'value': a['value'][0], 'baseline': a['baseline']}
    return _INPUT[key]


def lift(a):
    """the world points of the valid pixels of every frame, float64 (m, 3)"""
    disp = a['disp'].astype(np.float64)
    tl, H, W = disp.shape
    K = a['K'].astype(np.float64)
    pts = []
    for f in range(tl):
        ok = np.isfinite(disp[f]) & (disp[f] > 0)
        v, u = np.nonzero(ok)
        z = K[0, 0] * float(a['baseline']) / disp[f][v, u]
        P = np.stack([z * (u - K[0, 2]) / K[0, 0], z * (v - K[1, 2]) / K[1, 1], z], 1)
        pts.append((P - a['t'][f].astype(np.float64)) @ a['R'][f].astype(np.float64))     # R^T (P - t)
    return np.concatenate(pts)


def volume(shape, kind, grid):
    """-> (origin (3) float32, voxel, trunc): origin at the 1st percentile of the lifted points, the voxel the largest of
    (99th - 1st percentile) / (n - 1) over the axes, trunc = 3 voxels"""
    key = (shape, kind, grid)
    if key not in _VOLUME:
        X = lift(make_input(shape, kind))
        lo, hi = np.percentile(X, 1, axis=0), np.percentile(X, 99, axis=0)
        voxel = float(np.float32(max((hi[k] - lo[k]) / (grid[k] - 1) for k in range(3))))
        _VOLUME[key] = (lo.astype(np.float32), voxel, float(np.float32(3 * voxel)))
    return _VOLUME[key]


def refs(shape, kind, grid):
    """(float32 restatement, float64 restatement, exempt points, exempt pairs): computed once per case and never changed"""
    key = (shape, kind, grid)
    if key not in _REF:
        a = make_input(shape, kind)
        origin, voxel, trunc = volume(shape, kind, grid)
        r32, r64 = (tsdf_ref.integrate(a['disp'], a['R'], a['t'], a['K'], a['baseline'], a['value'], origin, voxel, trunc, grid, dtype=dt)
                    for dt in (np.float32, np.float64))
        ex, ex_pairs = tsdf_ref.exempt(r32, r64)
        _REF[key] = (r32, r64, ex, ex_pairs)
    return _REF[key]
