"""Mesh-scene training tracks rendered on the device: scenes with depth discontinuities, occlusion and projector shadows.

The recipe is the reference's data/create_syn_data.py (get_mesh :106-144, create_data :147-189) without ShapeNet and without
connecting_the_dots' renderer: a large background board, four foreground objects from the procedural library of meshes.py, `tl` cameras
that jitter around a base offset and look at (0, 0, 3).  ops.render_track (csrc/render.hip) casts the rays; the image formation is
fixed in include/dis_hip.h, section "track rendering".  The flows are the exact rigid flows of the visible surface points (the
reference estimates them with LiteFlowNet).

    python -m depthinspace_amd.data.render ROOT --n N [--seed S] [--pattern default|real] [--pack] [--sgm [NDISP]]
"""
import argparse
import os

import numpy as np
import torch

from .. import synth
from . import meshes

TARGET = np.array([0.0, 0.0, 3.0])
BLEND = 0.6
BOARD_EXTENT = 500.0


def random_rotation(rng):
    """uniformly distributed rotation matrix from three uniform draws (unit quaternion by the subgroup algorithm)"""
    u1, u2, u3 = rng.uniform(0, 1, 3)
    a, b = np.sqrt(1.0 - u1), np.sqrt(u1)
    x, y, z, w = a * np.sin(2 * np.pi * u2), a * np.cos(2 * np.pi * u2), b * np.sin(2 * np.pi * u3), b * np.cos(2 * np.pi * u3)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def board(z, extent=BOARD_EXTENT):
    """the background: two triangles, normal towards the cameras (-z).  The reference scales the board's depth spread about its
    mean by 500, but its board is a plane of constant z, so the spread - the 'tilt' - is zero; the look-at rotation of the cameras is
    what inclines it in the images."""
    v = np.array([[-extent, -extent, z], [extent, -extent, z], [extent, extent, z], [-extent, extent, z]], dtype=np.float64)
    return v, np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32)


def sample_scene(rng, objects=None, n_objects=4):
    """-> verts (nv, 3) float32 world coordinates, faces (nf, 3) int32, albedo (nf) float32.
    A board at z in [3, 5] with +-500 extent and a uniform grey, then n_objects foreground objects drawn from `objects` (meshes inside
    [-1, 1]^3; default: meshes.default_objects()): scale U(0.25, 1), uniform random rotation, nearest point at z = U(0.5, 3), xy shift
    U(-1, 1)^2, a uniform grey each."""
    if objects is None:
        objects = meshes.default_objects()
    parts = [board(rng.uniform(3, 5))]
    greys = [rng.uniform(0, 1)]
    for _ in range(n_objects):
        v, f = objects[rng.randint(0, len(objects))]
        v = np.asarray(v, dtype=np.float64) * rng.uniform(0.25, 1)
        v = v @ random_rotation(rng).T
        v[:, 2] += -v[:, 2].min() + rng.uniform(0.5, 3)
        v[:, :2] += rng.uniform(-1, 1, size=(1, 2))
        parts.append((v, f))
        greys.append(rng.uniform(0, 1))
    verts, faces = meshes.stack(parts)
    albedo = np.concatenate([np.full(len(f), g) for (_, f), g in zip(parts, greys)])
    return verts.astype(np.float32), faces.astype(np.int32), albedo.astype(np.float32)


def look_at(centre, target=TARGET):
    """R, t of a camera at `centre` whose optical axis passes through `target`, in the convention X_c = R X_w + t"""
    z = np.asarray(target, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 0)
    return R, -R @ np.asarray(centre, dtype=np.float64)


def sample_poses(rng, tl=4):
    """-> R (tl, 3, 3), t (tl, 3) float32 and the blend factor of the track: camera centres = a base offset U(-0.2, 0.2)^3 plus a
    per-frame jitter U(-0.1, 0.1)^3, each camera looking at (0, 0, 3); blend = clip(0.6 + U(-0.1, 0.1), 0, 1)."""
    base = rng.uniform(-0.2, 0.2, 3)
    blend = float(np.clip(BLEND + rng.uniform(-0.1, 0.1), 0, 1))
    Rs, ts = [], []
    for _ in range(tl):
        R, t = look_at(base + rng.uniform(-0.1, 0.1, 3))
        Rs.append(R)
        ts.append(t)
    return np.stack(Rs).astype(np.float32), np.stack(ts).astype(np.float32), blend


def sample_track(index, tl=4, seed=0, objects=None):
    """scene, poses and blend of track `index`: one generator per track, seeded with seed + index"""
    rng = np.random.RandomState((int(seed) + int(index)) % (2 ** 31))
    verts, faces, albedo = sample_scene(rng, objects)
    R, t, blend = sample_poses(rng, tl)
    return verts, faces, albedo, R, t, blend


def _default_device():
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


def render_sampled(settings, index, tl=4, seed=0, objects=None, device=None, pattern=None, want_ids=False):
    """track `index` through ops.render_track -> (its dict of tensors, R, t) with R, t float32 numpy"""
    from .. import ops
    device = _default_device() if device is None else device
    verts, faces, albedo, R, t, blend = sample_track(index, tl, seed, objects)
    if pattern is None:
        pattern = torch.from_numpy(np.ascontiguousarray(settings.pattern[..., 0], dtype=np.float32)).to(device)
    up = lambda a: torch.from_numpy(a).to(device)
    res = ops.render_track(up(verts), up(faces), up(albedo), up(R), up(t), np.asarray(settings.K, dtype=np.float32),
                           settings.baseline, blend, pattern, want_ids=want_ids)
    return res, R, t


def render_batch(settings, bs, tl=4, seed=0, objects=None, device=None):
    """`bs` rendered tracks (track b is sample_track(b, tl, seed)) in the loader layout (bs, tl, ...) on the device: im0, ambient0,
    disp0 (bs, tl, 1, H, W), R (bs, tl, 3, 3), t (bs, tl, 3), flow_ij (bs, 1, 2, H, W) - what Worker.copy_data takes."""
    device = _default_device() if device is None else device
    pattern = torch.from_numpy(np.ascontiguousarray(settings.pattern[..., 0], dtype=np.float32)).to(device)
    objects = meshes.default_objects() if objects is None else objects
    tracks = [render_sampled(settings, b, tl, seed, objects, device, pattern) for b in range(bs)]
    as_t = lambda a: torch.as_tensor(a).to(device)
    out = {'im0': torch.stack([as_t(r['im']) for r, _, _ in tracks]), 'ambient0': torch.stack([as_t(r['ambient']) for r, _, _ in tracks]),
           'disp0': torch.stack([as_t(r['disp']) for r, _, _ in tracks]),
           'R': torch.stack([as_t(R) for _, R, _ in tracks]), 't': torch.stack([as_t(t) for _, _, t in tracks])}
    for i in range(tl):
        for j in range(tl):
            if i != j:
                out[f'flow_{i}{j}'] = torch.stack([as_t(r['flow'])[i * tl + j][None] for r, _, _ in tracks])
    return out


def write_rendered_dataset(root, settings, n, tl=4, seed=0, pack=False, objects=None, device=None, sgm=None):
    """Writes tracks 0 .. n - 1 (track i is sample_track(i, tl, seed)) in the on-disk schema of data/dataset.py: settings.npz,
    %08d/frames.npz (im, ambient, grad = zeros, disp (tl, 1, H, W), R, t) and %08d/flow.npz (flow_ij (1, 2, H, W)).  Incremental: a
    track whose two files exist is left alone.  pack: also (re)writes the packed files (data/packed.py).  The training readers expect
    tl = 4.  sgm: a candidate count (64, 128 or 256) also stores sgm_disp, the semi-global match of every frame against the pattern
    (ops.sgm_disparity, the call of data/presave_sgm.py); None: the files are what they were without it.  Returns the track
    directories."""
    from . import dataset as D
    root = str(root)
    D.save_settings(root, settings)
    device = _default_device() if device is None else device
    pattern = torch.from_numpy(np.ascontiguousarray(settings.pattern[..., 0], dtype=np.float32)).to(device)
    objects = meshes.default_objects() if objects is None else objects
    to_np = lambda a: np.ascontiguousarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float32)
    paths = []
    for i in range(n):
        d = os.path.join(root, f'{i:08d}')
        paths.append(d)
        if os.path.exists(os.path.join(d, 'frames.npz')) and os.path.exists(os.path.join(d, 'flow.npz')):
            continue
        os.makedirs(d, exist_ok=True)
        res, R, t = render_sampled(settings, i, tl, seed, objects, device, pattern)
        im, flow = to_np(res['im']), to_np(res['flow'])
        # flow.npz first: frames.npz is what marks a track directory as complete for the readers
        np.savez(os.path.join(d, 'flow.npz'), **{f'flow_{a}{b}': flow[a * tl + b][None] for a in range(tl) for b in range(tl) if a != b})
        extra = {}
        if sgm is not None:
            from .. import ops
            extra['sgm_disp'] = to_np(ops.sgm_disparity(res['im'], pattern, int(sgm)))
        np.savez(os.path.join(d, 'frames.npz'), im=im, ambient=to_np(res['ambient']), grad=np.zeros_like(im), disp=to_np(res['disp']),
                 R=R, t=t, **extra)
    if pack:
        from . import packed
        packed.pack_dataset(root)
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m depthinspace_amd.data.render', description=__doc__.split('\n')[0])
    ap.add_argument('root')
    ap.add_argument('--n', type=int, required=True, help='number of tracks')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--pattern', choices=['default', 'real'], default='default')
    ap.add_argument('--pack', action='store_true', help='also write the packed files (data/packed.py)')
    ap.add_argument('--sgm', type=int, nargs='?', const=64, default=None, choices=[64, 128, 256], metavar='NDISP',
                    help='also store sgm_disp, the semi-global match against the pattern (data/presave_sgm.py), with NDISP candidates')
    a = ap.parse_args(argv)
    paths = write_rendered_dataset(a.root, synth.make_settings(pattern=a.pattern), a.n, seed=a.seed, pack=a.pack, sgm=a.sgm)
    print(f'{len(paths)} tracks under {a.root}')


if __name__ == '__main__':
    main()
