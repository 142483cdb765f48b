"""Procedural triangle meshes for the track renderer (data/render.py): host-side numpy, no files needed.

Every primitive is CLOSED and consistently oriented: each edge is shared by exactly two faces that run through it in opposite
directions, normals point outwards (positive signed volume), and a vertex shared by several faces is ONE row of `verts` - the
renderer's edge rule is watertight for such meshes.  A mesh is a pair (verts (nv, 3) float64, faces (nf, 3) int32).  Primitives
are centred on the origin; `normalized` fits a mesh into the cube [-1, 1]^3, the size the scene sampler expects.  Composites are
several closed parts that reach into each other (never coincident faces), so that scenes have thin parts and concavities.

The reference draws its foreground objects from ShapeNet chairs (data/create_syn_data.py:77-103); this library stands in for them.
"""
import numpy as np


def _mesh(verts, faces):
    return np.ascontiguousarray(verts, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int32)


def signed_volume(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def weld(verts, faces, decimals=9):
    """merge vertices with equal (rounded) coordinates; drops nothing else"""
    key = np.round(np.asarray(verts, dtype=np.float64), decimals) + 0.0
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    return _mesh(uniq, inv.reshape(-1)[np.asarray(faces)])


def stack(meshes):
    """several meshes as one: vertices concatenated, the faces of mesh k offset by the vertex count of meshes 0 .. k - 1"""
    verts, faces, off = [], [], 0
    for v, f in meshes:
        verts.append(np.asarray(v, dtype=np.float64))
        faces.append(np.asarray(f, dtype=np.int64) + off)
        off += len(v)
    return _mesh(np.concatenate(verts, 0), np.concatenate(faces, 0))


def transformed(mesh, scale=1.0, rotation=None, shift=(0.0, 0.0, 0.0)):
    v = np.asarray(mesh[0], dtype=np.float64) * np.asarray(scale, dtype=np.float64)
    if rotation is not None:
        v = v @ np.asarray(rotation, dtype=np.float64).T
    return _mesh(v + np.asarray(shift, dtype=np.float64), mesh[1])


def normalized(mesh):
    """centred, largest extent 2: inside [-1, 1]^3"""
    v = np.asarray(mesh[0], dtype=np.float64)
    lo, hi = v.min(0), v.max(0)
    return _mesh((v - 0.5 * (lo + hi)) / (0.5 * (hi - lo).max()), mesh[1])


def subdivide(mesh, levels=1):
    """every triangle -> 4 through its edge midpoints; a midpoint is one vertex for both faces of the edge"""
    verts = [tuple(p) for p in np.asarray(mesh[0], dtype=np.float64).tolist()]
    faces = np.asarray(mesh[1], dtype=np.int64)
    for _ in range(levels):
        mid, out = {}, []

        def m(i, j):
            k = (i, j) if i < j else (j, i)
            if k not in mid:
                a, b = verts[i], verts[j]
                verts.append(((a[0] + b[0]) / 2, (a[1] + b[1]) / 2, (a[2] + b[2]) / 2))
                mid[k] = len(verts) - 1
            return mid[k]
        for a, b, c in faces.tolist():
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = np.asarray(out, dtype=np.int64)
    return _mesh(np.asarray(verts), faces)


def box(size=(1.0, 1.0, 1.0), n=1):
    """axis-aligned box, n x n quads per side"""
    verts, faces = [], []
    g = np.arange(n + 1) / n - 0.5
    for a in range(3):
        ua, va = (a + 1) % 3, (a + 2) % 3
        for s in (1.0, -1.0):
            base = len(verts)
            for j in range(n + 1):
                for i in range(n + 1):
                    p = [0.0, 0.0, 0.0]
                    p[a], p[ua], p[va] = 0.5 * s, g[i], g[j]
                    verts.append(p)
            for j in range(n):
                for i in range(n):
                    p00, p10 = base + j * (n + 1) + i, base + j * (n + 1) + i + 1
                    p01, p11 = p00 + n + 1, p10 + n + 1
                    quad = [(p00, p10, p11), (p00, p11, p01)]     # e_u x e_v = +e_a
                    faces += quad if s > 0 else [(x, z, y) for x, y, z in quad]
    v, f = weld(np.asarray(verts), np.asarray(faces))
    return _mesh(v * np.asarray(size, dtype=np.float64), f)


def icosphere(subdivisions=2, radius=1.0):
    """icosahedron (20 faces) subdivided `subdivisions` times onto the sphere: 20 * 4^s faces"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
                  (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)], dtype=np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(subdivisions):
        v, f = subdivide((v, f), 1)
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return _mesh(v * radius, f)


def _ring(n, radius, z):
    a = 2.0 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], 1)


def cylinder(radius=0.5, height=1.0, segments=24, stacks=1):
    verts = [_ring(segments, radius, height * (k / stacks - 0.5)) for k in range(stacks + 1)]
    verts += [np.array([[0.0, 0.0, -0.5 * height]]), np.array([[0.0, 0.0, 0.5 * height]])]
    cb, ct = (stacks + 1) * segments, (stacks + 1) * segments + 1
    faces = []
    for k in range(stacks):
        for i in range(segments):
            b0, b1 = k * segments + i, k * segments + (i + 1) % segments
            t0, t1 = b0 + segments, b1 + segments
            faces += [(b0, b1, t1), (b0, t1, t0)]
    top = stacks * segments
    for i in range(segments):
        j = (i + 1) % segments
        faces += [(cb, j, i), (ct, top + i, top + j)]
    return _mesh(np.concatenate(verts, 0), np.asarray(faces))


def cone(radius=0.5, height=1.0, segments=24):
    verts = np.concatenate([_ring(segments, radius, -0.5 * height), [[0.0, 0.0, -0.5 * height]], [[0.0, 0.0, 0.5 * height]]], 0)
    cb, apex = segments, segments + 1
    faces = []
    for i in range(segments):
        j = (i + 1) % segments
        faces += [(i, j, apex), (cb, j, i)]
    return _mesh(verts, np.asarray(faces))


def torus(major=0.7, minor=0.25, segments=24, sides=12):
    a = 2.0 * np.pi * np.arange(segments) / segments
    b = 2.0 * np.pi * np.arange(sides) / sides
    A, B = np.meshgrid(a, b, indexing='ij')
    r = major + minor * np.cos(B)
    verts = np.stack([r * np.cos(A), r * np.sin(A), minor * np.sin(B)], -1).reshape(-1, 3)
    faces = []
    for i in range(segments):
        for j in range(sides):
            p00, p10 = i * sides + j, ((i + 1) % segments) * sides + j
            p01, p11 = i * sides + (j + 1) % sides, ((i + 1) % segments) * sides + (j + 1) % sides
            faces += [(p00, p10, p11), (p00, p11, p01)]
    return _mesh(verts, np.asarray(faces))


def table():
    """a slab on four cylinder legs (the legs reach into the slab)"""
    parts = [transformed(box((1.6, 1.0, 0.12), n=2), shift=(0, 0, 0.5))]
    for sx in (-0.65, 0.65):
        for sy in (-0.38, 0.38):
            parts.append(transformed(cylinder(0.06, 1.0, segments=12), shift=(sx, sy, 0.0)))
    return stack(parts)


def chair():
    """seat, back rest and four square legs"""
    parts = [transformed(box((0.9, 0.9, 0.1), n=2), shift=(0, 0, 0.0)),
             transformed(box((0.9, 0.1, 1.0), n=2), shift=(0, 0.4, 0.45))]
    for sx in (-0.38, 0.38):
        for sy in (-0.38, 0.38):
            parts.append(transformed(box((0.09, 0.09, 0.8)), shift=(sx, sy, -0.38)))
    return stack(parts)


def bracket():
    """an L of two slabs with a cylinder through the upright one"""
    return stack([transformed(box((1.2, 0.8, 0.15), n=2), shift=(0, 0, -0.4)),
                  transformed(box((0.15, 0.8, 1.0), n=2), shift=(-0.5, 0, 0.05)),
                  transformed(cylinder(0.12, 0.9, segments=16), rotation=[[0, 0, 1], [0, 1, 0], [-1, 0, 0]], shift=(-0.5, 0, 0.2))])


def frame():
    """four bars around an opening: a concavity the background shows through"""
    return stack([transformed(box((1.6, 0.15, 0.15)), shift=(0, 0.55, 0)), transformed(box((1.6, 0.15, 0.15)), shift=(0, -0.55, 0)),
                  transformed(box((0.15, 1.2, 0.14)), shift=(0.72, 0, 0)), transformed(box((0.15, 1.2, 0.14)), shift=(-0.72, 0, 0))])


# name -> constructor with the default tessellation
LIBRARY = {'box': lambda: box(n=2), 'icosphere': lambda: icosphere(2), 'cylinder': lambda: cylinder(0.4, 1.4), 'cone': cone,
           'torus': torus, 'table': table, 'chair': chair, 'bracket': bracket, 'frame': frame}


def default_objects():
    """the library at its default tessellation, each mesh fitted into [-1, 1]^3, in the order of sorted names"""
    return [normalized(LIBRARY[k]()) for k in sorted(LIBRARY)]


def load_mesh(path):
    """a user mesh from an .npz with `verts` (nv, 3) and `faces` (nf, 3)"""
    with np.load(path) as f:
        verts, faces = np.asarray(f['verts'], dtype=np.float64), np.asarray(f['faces'])
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f'{path}: verts (nv, 3) and faces (nf, 3) are expected, got {verts.shape} and {faces.shape}')
    if len(faces) == 0 or faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError(f'{path}: a face index lies outside the {len(verts)} vertices')
    return _mesh(verts, faces)
