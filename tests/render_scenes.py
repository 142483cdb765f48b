"""Scenes and cameras shared by the renderer's tests (tests/test_render_cpu.py, tests/test_render_gpu.py)."""
import numpy as np

from depthinspace_amd import synth
from depthinspace_amd.data import meshes, render

SMALL_H, SMALL_W = 64, 48
SMALL_BASELINE = 0.2   # wide, so that projector shadows are several pixels across at this resolution


def small_settings(h=SMALL_H, w=SMALL_W, baseline=SMALL_BASELINE):
    """the default camera scaled by 1/8 (fx = fy = 54.4) with the principal point at the image centre, default pattern crop"""
    s = synth.make_settings(h, w)
    K = np.array([[54.4 * w / SMALL_W, 0, (w - 1) / 2.0], [0, 54.4 * w / SMALL_W, (h - 1) / 2.0], [0, 0, 1]], dtype=np.float32)
    return synth.Settings((h, w), K, baseline, s.pattern)


def _placed(rng, mesh, scale, z_near, xy):
    v = np.asarray(mesh[0]) * scale
    v = v @ render.random_rotation(rng).T
    v[:, 2] += -v[:, 2].min() + z_near
    v[:, :2] += np.asarray(xy)
    return v, mesh[1]


def small_scene(seed, tl=3):
    """a board, two rotated boxes and one 20-face icosahedron: 46 triangles -> verts, faces, albedo, R, t, blend"""
    rng = np.random.RandomState(seed)
    parts = [render.board(rng.uniform(3, 4)),
             _placed(rng, meshes.box(), rng.uniform(0.7, 1.0), rng.uniform(1.4, 2.0), rng.uniform(-0.5, 0.0, 2)),
             _placed(rng, meshes.box(), rng.uniform(0.5, 0.8), rng.uniform(1.8, 2.4), rng.uniform(0.0, 0.5, 2)),
             _placed(rng, meshes.icosphere(0), rng.uniform(0.3, 0.5), rng.uniform(1.2, 1.8), rng.uniform(-0.4, 0.4, 2))]
    verts, faces = meshes.stack(parts)
    albedo = np.concatenate([np.full(len(f), g) for (_, f), g in zip(parts, rng.uniform(0.3, 1.0, len(parts)))])
    R, t, blend = render.sample_poses(rng, tl)
    assert len(faces) == 46
    return verts.astype(np.float32), faces.astype(np.int32), albedo.astype(np.float32), R, t, blend


def plane_scene(settings, tl, seed):
    """two triangles in synth's plane  n . X = c  (far larger than the view) with the poses of synth.make_batch(scene='plane', seed)
    -> verts, faces, albedo, R, t and synth's batch"""
    batch = synth.make_batch(settings, 1, tl, seed=seed, with_primary=False)
    n, c = synth._PLANE_N, synth._PLANE_C
    xy = 40.0 * np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64)
    z = (c - xy @ n[:2]) / n[2]
    verts = np.concatenate([xy, z[:, None]], 1).astype(np.float64)
    faces = np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32)
    return verts, faces, np.full(2, 0.8, np.float32), batch['R'][0], batch['t'][0], batch


def dense_scene(seed=5):
    """about 5 000 triangles for a 96 x 80 image: subdivided primitives, some of them partly outside the frame, a far icosphere whose
    triangles are smaller than a pixel, and one small triangle 0.02 in front of the camera (nearer than the renderer's near
    distance, off the optical axis) -> verts, faces, albedo, R, t, blend"""
    rng = np.random.RandomState(seed)
    parts = [render.board(3.6),
             _placed(rng, meshes.box(n=8), 0.8, 1.6, (-0.45, -0.3)),                       # 768
             _placed(rng, meshes.torus(segments=32, sides=16), 0.7, 1.3, (0.35, 0.45)),     # 1024
             _placed(rng, meshes.cylinder(0.3, 1.6, segments=32, stacks=8), 1.0, 1.5, (0.9, -0.2)),   # 576, partly outside
             _placed(rng, meshes.icosphere(3), 0.08, 3.0, (0.1, -0.1)),                     # 1280 sub-pixel triangles
             _placed(rng, meshes.icosphere(3), 0.45, 1.0, (-0.75, 0.6))]                    # 1280, partly outside
    R, t, blend = render.sample_poses(rng, 1)
    # a small triangle 0.02 in front of camera 0: X_w = R^T (X_c - t)
    near_c = np.array([[0.004, 0.004, 0.02], [0.010, 0.004, 0.02], [0.004, 0.012, 0.02]])
    near_w = (near_c - t[0].astype(np.float64)) @ R[0].astype(np.float64)
    parts.append((near_w, np.array([[0, 1, 2]], dtype=np.int32)))
    verts, faces = meshes.stack(parts)
    albedo = np.concatenate([np.full(len(f), g) for (_, f), g in zip(parts, rng.uniform(0.3, 1.0, len(parts)))])
    return verts.astype(np.float32), faces.astype(np.int32), albedo.astype(np.float32), R, t, blend


def sphere_scene(subdivisions=2, radius=0.5, centre=(0.05, -0.03, 1.8), board_z=3.5):
    """an icosphere (20 * 4^s faces) in front of a board, one camera at the origin -> verts, faces, albedo, R, t, and the radius of
    the sphere inscribed in the mesh (the smallest distance of a face plane from the centre)"""
    v, f = meshes.icosphere(subdivisions, radius)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    r_in = float(np.min(np.sum(n * a, 1)))
    verts, faces = meshes.stack([render.board(board_z), (v + np.asarray(centre), f)])
    albedo = np.full(len(faces), 0.7, np.float32)
    return verts.astype(np.float32), faces.astype(np.int32), albedo, np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), r_in
