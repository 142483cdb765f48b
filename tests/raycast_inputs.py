"""Inputs and cached restatements shared by the raycast tests (tests/test_raycast_ref_cpu.py, tests/test_raycast_gpu.py): the cases of
tests/tsdf_inputs.py - every shape, every kind, every grid -, the volume being the FLOAT32 RESTATEMENT of the integration
(tsdf_ref.integrate through tsdf_inputs.refs), not the device's, cast into the track's own poses and one novel view at steps of
0.5, 1 and 2 voxels."""
import numpy as np

from tests import raycast_ref
from tests import tsdf_inputs as TI

KINDS = TI.KINDS
SHAPES = list(TI.SHAPES)
# a single cell; odd, less than one brick; bricks cut by the lattice's end; 5 x 5 x 6 bricks; 9 x 8 x 8 bricks, 1056 blocks of the state pass
GRIDS = [(2, 2, 2), (7, 3, 5), (33, 17, 20), (40, 40, 48), (66, 64, 64)]
STEPS = [0.5, 1.0, 2.0]          # in voxels

# The cases left out: their exempt share - in per cent of the case's pixels, measured by the restatement itself - breaks the cap of 0.5 %
# that tests/test_raycast_ref_cpu.py holds every case to.  The band that decides is the one around s = 0,
# tsdf_ref.tolerance(s32, s64): these inputs have long focal lengths (fx = 435 at 37 .. 96 pixels), so a lattice coordinate of some
# hundreds of voxels is formed from depths of 3 and voxels of 0.004 .. 0.01, float32 and float64 differ by up to 1e-4 of a voxel in
# it and by 2e-5 in s, and a ray whose s passes within 3e-4 .. 1.5e-3 of 0 at a sample is exempt; the share grows with the samples
# per voxel and with the lattice.
DROPPED = {
    ((2, 19, 37), 'plane', (33, 17, 20), 0.5): 0.5216,
    ((2, 19, 37), 'plane', (40, 40, 48), 0.5): 0.8535,
    ((2, 19, 37), 'plane', (66, 64, 64), 0.5): 1.1854,
    ((2, 19, 37), 'plane', (66, 64, 64), 1.0): 0.6164,
    ((2, 19, 37), 'bumps', (40, 40, 48), 0.5): 0.5216,
    ((2, 19, 37), 'bumps', (66, 64, 64), 0.5): 0.9483,
    ((2, 19, 37), 'noise', (33, 17, 20), 0.5): 0.6164,
    ((2, 19, 37), 'noise', (40, 40, 48), 0.5): 0.9483,
    ((2, 19, 37), 'noise', (66, 64, 64), 0.5): 2.5605,
    ((2, 19, 37), 'noise', (66, 64, 64), 1.0): 1.0431,
    ((2, 19, 37), 'noise', (66, 64, 64), 2.0): 0.6164,
    ((2, 19, 37), 'holes', (66, 64, 64), 0.5): 0.8061,
    ((3, 24, 40), 'plane', (40, 40, 48), 0.5): 0.5729,
    ((3, 24, 40), 'plane', (66, 64, 64), 0.5): 2.5000,
    ((3, 24, 40), 'plane', (66, 64, 64), 1.0): 0.5729,
    ((3, 24, 40), 'bumps', (40, 40, 48), 0.5): 0.9635,
    ((3, 24, 40), 'bumps', (66, 64, 64), 0.5): 0.8073,
    ((3, 24, 40), 'noise', (33, 17, 20), 0.5): 1.0677,
    ((3, 24, 40), 'noise', (40, 40, 48), 0.5): 1.1979,
    ((3, 24, 40), 'noise', (40, 40, 48), 1.0): 0.7812,
    ((3, 24, 40), 'noise', (66, 64, 64), 0.5): 4.6094,
    ((3, 24, 40), 'noise', (66, 64, 64), 1.0): 0.9115,
    ((3, 24, 40), 'holes', (33, 17, 20), 0.5): 1.8750,
    ((3, 24, 40), 'holes', (40, 40, 48), 0.5): 0.5729,
    ((3, 24, 40), 'holes', (66, 64, 64), 0.5): 1.1198,
    ((3, 24, 40), 'holes', (66, 64, 64), 1.0): 0.6510,
    ((4, 64, 96), 'plane', (66, 64, 64), 0.5): 0.7259,
    ((4, 64, 96), 'plane', (66, 64, 64), 1.0): 0.5436,
    ((4, 64, 96), 'bumps', (66, 64, 64), 0.5): 0.7454,
    ((4, 64, 96), 'noise', (66, 64, 64), 0.5): 1.9434,
    ((4, 64, 96), 'noise', (66, 64, 64), 1.0): 0.7552,
    ((4, 64, 96), 'holes', (66, 64, 64), 0.5): 0.6934,
}


def steps(shape, kind, grid):
    """the steps, in voxels, at which the case is cast"""
    return [sv for sv in STEPS if (shape, kind, grid, sv) not in DROPPED]


_REF = {}


def grid_id(g):
    return 'x'.join(str(v) for v in g)


def novel_view(R0, t0, K, width, origin, voxel, grid):
    """frame 0's pose turned about the camera's y axis - by 6 degrees, or by the angle that moves the image by 0.4 of its width where
    that is less (a long focal length) - and moved along its x axis so that half of that turn is undone at the depth of the lattice's
    centre: X_c' = Rd X_c + td.  Part of the image then looks past the box"""
    a = min(np.deg2rad(6.0), np.arctan(0.4 * width / float(K[0][0])))
    Rd = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    centre = np.asarray(origin, dtype=np.float64) + (np.asarray(grid, dtype=np.float64) - 1) * float(voxel) / 2
    zc = float((R0.astype(np.float64) @ centre + t0.astype(np.float64))[2])
    td = np.array([-0.5 * zc * np.sin(a), 0.0, 0.0])
    return (Rd @ R0.astype(np.float64)).astype(np.float32), (Rd @ t0.astype(np.float64) + td).astype(np.float32)


def volume(shape, kind, grid):
    """-> dict tsdf, weight, vvalue (nz, ny, nx) of the float32 restatement, origin, voxel, trunc"""
    r32 = TI.refs(shape, kind, grid)[0]
    origin, voxel, trunc = TI.volume(shape, kind, grid)
    return {'tsdf': r32['tsdf'].astype(np.float32), 'weight': r32['weight'], 'vvalue': r32['vvalue'].astype(np.float32), 'origin': origin,
            'voxel': voxel, 'trunc': trunc}


def views(shape, kind, grid):
    """R (tl + 1, 3, 3), t (tl + 1, 3) float32: the track's own poses, then the novel view"""
    a = TI.make_input(shape, kind)
    origin, voxel, _ = TI.volume(shape, kind, grid)
    Rn, tn = novel_view(a['R'][0], a['t'][0], a['K'], shape[2], origin, voxel, grid)
    return np.concatenate([a['R'], Rn[None]]).astype(np.float32), np.concatenate([a['t'], tn[None]]).astype(np.float32)


def step_of(voxel, step_voxels):
    return float(np.float32(step_voxels * voxel))


def cast(shape, kind, grid, step_voxels, min_weight, dtype, R=None, t=None):
    a = TI.make_input(shape, kind)
    vol = volume(shape, kind, grid)
    if R is None:
        R, t = views(shape, kind, grid)
    return raycast_ref.cast(vol['tsdf'], vol['weight'], vol['vvalue'], vol['origin'], vol['voxel'], R, t, a['K'], a['baseline'], shape[1:],
                            step=step_of(vol['voxel'], step_voxels), min_weight=min_weight, dtype=dtype)


def refs(shape, kind, grid, step_voxels=1.0, min_weight=1):
    """(float32 restatement, float64 restatement, exempt pixels): computed once per case and never changed; the per-sample records are
    dropped once the exemption has been formed from them"""
    key = (shape, kind, grid, step_voxels, min_weight)
    if key not in _REF:
        r32, r64 = (cast(shape, kind, grid, step_voxels, min_weight, dt) for dt in (np.float32, np.float64))
        ex = raycast_ref.exempt(r32, r64)
        del r32['views'], r64['views']
        _REF[key] = (r32, r64, ex)
    return _REF[key]
