"""Inputs and cached restatements shared by the frame-to-model alignment tests (tests/test_tsdf_align_ref_cpu.py,
tests/test_tsdf_align_gpu.py): the cases of tests/tsdf_inputs.py, the volume being the FLOAT32 RESTATEMENT of the integration
(raycast_inputs.volume).  The views of a case are the track's own frames (`track`, nv = tl), one of them (`one`, nv = 1: view 1 of
`many`) or the frames twice plus raycast_inputs.novel_view, whose disparities are the float32 raycast restatement's (`many`,
nv = 2 tl + 1, every view with a start of its own).  A start is the true pose moved on the left by a fixed twist: `mag` voxels of
translation along a fixed direction per view, and a rotation that moves the lattice's centre by `mag` voxels."""
import numpy as np

from tests import raycast_inputs as RI
from tests import tsdf_align_ref
from tests import tsdf_inputs as TI

KINDS = TI.KINDS
SHAPES = list(TI.SHAPES)
# a single cell, in which no pixel is used: every view fails and returns its start; and a lattice whose voxel is a seventh of the scene, on
# which some views are used, some fail in a later pass and keep their last good state
FAIL_GRIDS = [(2, 2, 2), (7, 3, 5)]
GRIDS = [(33, 17, 20), (40, 40, 48), (66, 64, 64)]
MODES = ['track', 'one', 'many']
# (iters, scale, damping) with scale None, 'trunc' or 'trunc/4'
PARAMS = [(6, None, 0.0), (3, 'trunc', 1e-3), (12, 'trunc/4', 0.0)]

# fixed unit directions, one per view index
_DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [1, -1, 0], [0, 1, -1], [-1, 0, 1]], np.float64)
_DIRS /= np.linalg.norm(_DIRS, axis=1, keepdims=True)

_REF, _VIEWS = {}, {}
_ALL = GRIDS + FAIL_GRIDS


def mode_of(shape, kind, grid):
    """a case is a shape, a kind and a grid; it has one view mode and one parameter set, and both go round the cases, each in its own
    way, so that every shape, kind and grid meets all three of either"""
    return MODES[(SHAPES.index(shape) + KINDS.index(kind) + _ALL.index(grid)) % len(MODES)]


def case_params(shape, kind, grid):
    return PARAMS[(SHAPES.index(shape) + 2 * KINDS.index(kind) + 2 * _ALL.index(grid)) % len(PARAMS)]


def scale_of(name, trunc):
    return {None: None, 'trunc': trunc, 'trunc/4': float(np.float32(trunc / 4))}[name]


def perturb(R, t, centre, voxel, index, mag=0.5):
    """the pose (R, t) moved on the left: R' = dR R, t' = dR t + delta, delta = mag voxel along direction `index`, dR a rotation about
    the axis across that direction and the line of sight to `centre` (a world point) by the angle that moves `centre` by mag voxel"""
    R, t = R.astype(np.float64), t.astype(np.float64)
    c = R @ np.asarray(centre, dtype=np.float64) + t
    dirn = _DIRS[index % len(_DIRS)]
    ax = np.cross(c, dirn)
    if np.linalg.norm(ax) < 1e-9 * np.linalg.norm(c):
        ax = np.cross(c, _DIRS[(index + 1) % len(_DIRS)])
    ax /= np.linalg.norm(ax)
    ang = mag * float(voxel) / np.linalg.norm(c)
    Wx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    dR = np.eye(3) + np.sin(ang) * Wx + (1 - np.cos(ang)) * (Wx @ Wx)
    return (dR @ R).astype(np.float32), (dR @ t + mag * float(voxel) * dirn).astype(np.float32)


def centre_of(origin, voxel, grid):
    return np.asarray(origin, dtype=np.float64) + (np.asarray(grid, dtype=np.float64) - 1) * float(voxel) / 2


def views(shape, kind, grid, mode, mag=0.5):
    """-> dict disp (nv, H, W), R_true, t_true, R_init, t_init float32"""
    key = (shape, kind, grid, mode, mag)
    if key in _VIEWS:
        return _VIEWS[key]
    a = TI.make_input(shape, kind)
    origin, voxel, _ = TI.volume(shape, kind, grid)
    tl = shape[0]
    if mode == 'track':
        disp, R, t, idx = a['disp'], a['R'], a['t'], list(range(tl))
    else:
        Rn, tn = RI.novel_view(a['R'][0], a['t'][0], a['K'], shape[2], origin, voxel, grid)
        dn = RI.cast(shape, kind, grid, 1.0, 1, np.float32, R=Rn[None], t=tn[None])['disp'].astype(np.float32)
        disp = np.concatenate([a['disp'], a['disp'], dn])
        R, t = np.concatenate([a['R'], a['R'], Rn[None]]), np.concatenate([a['t'], a['t'], tn[None]])
        idx = list(range(1, 2 * tl + 2))                           # (the second copy of a frame starts elsewhere than the first)
        if mode == 'one':
            disp, R, t, idx = disp[1:2], R[1:2], t[1:2], idx[1:2]
    centre = centre_of(origin, voxel, grid)
    starts = [perturb(R[k], t[k], centre, voxel, idx[k], mag) for k in range(len(R))]
    _VIEWS[key] = {'disp': np.ascontiguousarray(disp, dtype=np.float32), 'R_true': R.astype(np.float32), 't_true': t.astype(np.float32),
                   'R_init': np.stack([s[0] for s in starts]), 't_init': np.stack([s[1] for s in starts])}
    return _VIEWS[key]


def run(shape, kind, grid, mode, dtype, params=None, min_weight=1, mag=0.5):
    a = TI.make_input(shape, kind)
    vol = RI.volume(shape, kind, grid)
    v = views(shape, kind, grid, mode, mag)
    iters, scale, damping = case_params(shape, kind, grid) if params is None else params
    return tsdf_align_ref.align(vol['tsdf'], vol['weight'], vol['origin'], vol['voxel'], vol['trunc'], v['disp'], a['K'], a['baseline'],
                                v['R_init'], v['t_init'], iters=iters, scale=scale_of(scale, vol['trunc']), damping=damping,
                                min_weight=min_weight, dtype=dtype)


def refs(shape, kind, grid):
    """(float32 restatement, float64 restatement): computed once per case and never changed"""
    key = (shape, kind, grid)
    if key not in _REF:
        _REF[key] = tuple(run(shape, kind, grid, mode_of(shape, kind, grid), dt) for dt in (np.float32, np.float64))
    return _REF[key]


def counts(r):
    """the outputs that must be equal: pixels used (both passes), status, valid disparities"""
    return r['stats'][:, [0, 3, 4, 7]].astype(np.float64)


def float_outputs(r):
    """the outputs that are compared within pose_ref.tolerance, each on its own, as tests/test_pose_gpu.py does"""
    return (('R', r['R']), ('t', r['t']), ('mean weight', r['stats'][:, [1, 5]]), ('rms residual', r['stats'][:, [2, 6]]))


def cap_tolerance(r32, r64):
    """the larger of the tolerances of R and t: what the cap of 1e-4 is held against, as in tests/test_pose_ref_cpu.py"""
    return max(tsdf_align_ref.tolerance(r32[k], r64[k]) for k in ('R', 't'))


# The cases left out: the tolerance of R or t - pose_ref.tolerance, measured by the restatement itself - breaks the cap of 1e-4 that
# tests/test_tsdf_align_ref_cpu.py holds every case to, or the two restatements disagree on a count (a pixel at the edge of the band
# |s| < 1, of a cell or of the lattice falls either way).  -> (the measured tolerance, the counts agree).  The near-planar kinds slide
# along the directions their surface does not constrain, where the rounding of a lattice coordinate - formed from depths of 3 and
# voxels of 0.004 .. 0.02 - is amplified; on the 7 x 3 x 5 lattice a voxel is a seventh of the scene and a start half a voxel off is far.
DROPPED = {
    ((2, 19, 37), 'plane', (40, 40, 48)): (4.488e-03, False),
    ((2, 19, 37), 'plane', (7, 3, 5)): (5.446e+00, False),
    ((2, 19, 37), 'noise', (7, 3, 5)): (1.404e-04, True),
    ((2, 19, 37), 'holes', (7, 3, 5)): (1.786e+01, False),
    ((3, 24, 40), 'plane', (40, 40, 48)): (1.309e-04, True),
    ((3, 24, 40), 'plane', (7, 3, 5)): (4.759e-01, False),
    ((3, 24, 40), 'bumps', (40, 40, 48)): (1.448e-02, False),
    ((3, 24, 40), 'bumps', (7, 3, 5)): (7.212e-03, True),
    ((3, 24, 40), 'noise', (33, 17, 20)): (5.530e-03, True),
    ((3, 24, 40), 'holes', (40, 40, 48)): (1.850e-04, True),
    ((3, 24, 40), 'holes', (7, 3, 5)): (5.406e-01, False),
    ((4, 64, 96), 'plane', (33, 17, 20)): (6.105e-03, False),
    ((4, 64, 96), 'bumps', (66, 64, 64)): (1.807e-05, False),
    ((4, 64, 96), 'bumps', (7, 3, 5)): (6.277e+01, True),
    ((4, 64, 96), 'noise', (40, 40, 48)): (1.021e-04, False),
    ((4, 64, 96), 'noise', (66, 64, 64)): (2.145e-04, True),
    ((4, 64, 96), 'noise', (7, 3, 5)): (2.868e+00, False),
    ((4, 64, 96), 'holes', (33, 17, 20)): (4.534e-03, False),
}


ALL_GRIDS = GRIDS + FAIL_GRIDS


def cases(grids=None):
    return [(s, k, g) for s in SHAPES for k in KINDS for g in (ALL_GRIDS if grids is None else grids)]


def kept(grids=None):
    return [c for c in cases(grids) if c not in DROPPED]


def case_id(c):
    s, k, g = c
    return f'{TI.shape_id(s)}-{k}-{RI.grid_id(g)}-{mode_of(s, k, g)}'
