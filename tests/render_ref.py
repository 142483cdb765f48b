"""Test oracle of the track renderer: the image formation of include/dis_hip.h, section "track rendering", in numpy - and nothing else.

Brute force: every ray against every triangle with Moeller-Trumbore (Cramer's rule on  o + t d = A + u e1 + v e2).  All primary rays
of a frame leave the camera centre and all its shadow rays end in the projector centre, so with that point as the origin `o` the
three determinants are dot products of the ray direction with one vector per triangle, and rays x triangles is three matrix
products.  dtype = float64 is the oracle; dtype = float32 runs the same arithmetic in single precision and gives the tests their
error scale.
"""
import numpy as np

KA, KD = 0.5, 1.5
SHADOW_EPS = 1e-4


def _mt(origin, dirs, A, B, C):
    """rays origin + t dirs[n] against triangles (A, B, C)[k] -> t (n, k), inf where the ray misses (u, v >= 0, u + v <= 1)"""
    e1, e2, tv = B - A, C - A, origin[None] - A
    q = np.cross(tv, e1)
    with np.errstate(divide='ignore', invalid='ignore'):
        det = dirs @ np.cross(e2, e1).T
        u = (dirs @ np.cross(e2, tv).T) / det
        v = (dirs @ q.T) / det
        t = np.sum(e2 * q, 1)[None] / det
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    return np.where(ok, t, np.inf).astype(dirs.dtype)


def _bilinear_border(img, x, y):
    H, W = img.shape
    x = np.clip(x, 0, W - 1)
    y = np.clip(y, 0, H - 1)
    x0 = np.floor(x).astype(np.int64)
    y0 = np.floor(y).astype(np.int64)
    x1 = np.minimum(x0 + 1, W - 1)
    y1 = np.minimum(y0 + 1, H - 1)
    fx, fy = x - x0, y - y0
    return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


def render_frame(verts, faces, albedo, R, t, i, K, baseline, blend, pattern, u, v, dtype=np.float64, du=0.0, dv=0.0, ids_only=False,
                 visibility=True):
    """frame i at the pixels (u[n], v[n]) (ints), rays through (u + du, v + dv).  -> dict of (n, ...) arrays: tri_id, lit, and unless
    ids_only disp, ambient, im, flow (tl, 2, n), visible_in (tl, n): whether frame j's nearest surface along its ray to the point is
    the point itself (up to 1e-6 relative depth)."""
    f = dtype
    verts, albedo, R, t = verts.astype(f), albedo.astype(f), R.astype(f), t.astype(f)
    fx, fy, cx, cy = f(K[0, 0]), f(K[1, 1]), f(K[0, 2]), f(K[1, 2])
    b, blend = f(baseline), f(blend)
    Vc = verts @ R[i].T + t[i]
    A, B, C = Vc[faces[:, 0]], Vc[faces[:, 1]], Vc[faces[:, 2]]
    uu, vv = u.astype(f) + f(du), v.astype(f) + f(dv)
    d = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], 1)
    T = _mt(np.zeros(3, f), d, A, B, C)
    T = np.where(T > 0, T, np.inf)
    tid = np.argmin(T, 1)                      # the first minimum: the lower index on equal depth
    z = T[np.arange(len(tid)), tid]
    hit = np.isfinite(z)
    tid = np.where(hit, tid, -1)
    zs = np.where(hit, z, 1).astype(f)
    P = d * zs[:, None]
    cp = np.array([b, 0, 0], f)
    S = _mt(cp, P - cp[None], A, B, C)         # parameter 0 at the projector, 1 at the point
    S[np.arange(len(tid)), np.maximum(tid, 0)] = np.inf
    lit = hit & ~np.any((S > f(SHADOW_EPS)) & (S < f(1) - f(SHADOW_EPS)), 1)
    out = {'tri_id': tid.astype(np.int32), 'lit': lit.astype(np.float32)}
    if ids_only:
        return out
    k = np.maximum(tid, 0)
    n = np.cross(B[k] - A[k], C[k] - A[k])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), f(1e-300) if f is np.float64 else f(1e-30))
    c = -P / np.linalg.norm(P, axis=1, keepdims=True)
    n = np.where(np.sum(n * c, 1, keepdims=True) < 0, -n, n)
    p = cp[None] - P
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    g = albedo[k]
    disp = np.where(hit, b * fx / zs, 0)
    amb = np.clip(g * (f(KA) + f(KD) * np.maximum(0, np.sum(n * c, 1))) / 2, 0, 1)
    pat = _bilinear_border(pattern.astype(f), u.astype(f) - disp, v.astype(f))
    pr = np.clip(g * (f(KA) + f(KD) * np.maximum(0, np.sum(n * p, 1))) / 2, 0, 1) * pat * lit
    im = np.clip(blend * pr + (1 - blend) * amb, 0, 1)
    Xw = (P - t[i][None]) @ R[i]
    tl = len(R)
    flow = np.zeros((tl, 2, len(u)), f)
    vis = np.zeros((tl, len(u)), bool)
    for j in range(tl):
        if j == i:
            vis[j] = hit
            continue
        Xj = Xw @ R[j].T + t[j][None]
        with np.errstate(divide='ignore', invalid='ignore'):
            flow[j, 0] = np.where(hit, (fx * Xj[:, 0] / Xj[:, 2] + cx) - u.astype(f), 0)
            flow[j, 1] = np.where(hit, (fy * Xj[:, 1] / Xj[:, 2] + cy) - v.astype(f), 0)
            dj = Xj / Xj[:, 2:3]
        if not visibility:
            continue
        Vj = verts @ R[j].T + t[j]
        Tj = _mt(np.zeros(3, f), dj, Vj[faces[:, 0]], Vj[faces[:, 1]], Vj[faces[:, 2]])
        Tj = np.where(Tj > 0, Tj, np.inf)
        vis[j] = hit & (Xj[:, 2] > 0) & (np.abs(Tj.min(1) - Xj[:, 2]) <= 1e-6 * np.abs(Xj[:, 2]))
    out.update(disp=disp.astype(f), ambient=np.where(hit, amb, 0).astype(f), im=np.where(hit, im, 0).astype(f), flow=flow, visible_in=vis)
    return out


AMBIGUITY_OFFSETS = ((0.01, 0.0), (-0.01, 0.0), (0.0, 0.01), (0.0, -0.01))


def render_ref(verts, faces, albedo, R, t, K, baseline, blend, pattern, dtype=np.float64, pixels=None, ambiguity=True, visibility=True):
    """The whole track on the full image, or on `pixels` = (u, v) int arrays.  -> dict with a leading frame axis and a trailing pixel
    axis n (full image: n = h * w in row order): tri_id, lit, disp, ambient, im (tl, n), flow (tl, tl, 2, n), visible_in (tl, tl, n),
    and with `ambiguity` `ambiguous` (tl, n): the float64 triangle id or lit flag of the pixel differs between the centre ray and any
    of the four rays offset by +-0.01 px."""
    h, w = pattern.shape
    if pixels is None:
        vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        u, v = uu.reshape(-1), vv.reshape(-1)
    else:
        u, v = (np.asarray(p).reshape(-1) for p in pixels)
    faces = np.asarray(faces, dtype=np.int64)
    frames = [render_frame(verts, faces, albedo, R, t, i, K, baseline, blend, pattern, u, v, dtype, visibility=visibility)
              for i in range(len(R))]
    out = {k: np.stack([fr[k] for fr in frames]) for k in frames[0]}
    if ambiguity:
        amb = np.zeros(out['tri_id'].shape, bool)
        for i in range(len(R)):
            c = frames[i] if dtype is np.float64 else render_frame(verts, faces, albedo, R, t, i, K, baseline, blend, pattern, u, v,
                                                                   np.float64, ids_only=True)
            for du, dv in AMBIGUITY_OFFSETS:
                o = render_frame(verts, faces, albedo, R, t, i, K, baseline, blend, pattern, u, v, np.float64, du, dv, ids_only=True)
                amb[i] |= (o['tri_id'] != c['tri_id']) | (o['lit'] != c['lit'])
        out['ambiguous'] = amb
    return out
