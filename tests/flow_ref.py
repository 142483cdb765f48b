"""Numpy restatement of the dense optical flow (include/dis_hip.h, section "dense optical flow"): coarse-to-fine Horn-Schunck with
warping, every stage returned.  Parameterised by dtype: the same code runs in float64 (the reference) and in float32 (what the
kernels' arithmetic is; the distance between the two gives the tests their tolerance).  Every sum is written in an explicit operand
order, which csrc/flow.hip follows.  All pairs of all tracks are carried along a leading axis."""
import numpy as np


def pairs(tl):
    """the ordered pairs (i, j), i != j, in the order q = i (tl - 1) + (j - (j > i))"""
    return [(i, j) for i in range(tl) for j in range(tl) if j != i]


def level_sizes(h, w, min_size):
    """[(h_0, w_0), (h_1, w_1), ...]: a further level while min(h, w) >= 2 min_size at the coarsest; sizes halve with ceil"""
    out = [(h, w)]
    while min(out[-1]) >= 2 * min_size:
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def normalise(frames, dtype):
    """(..., H, W) float32 -> (I - mean) / max(std, 1e-6): population moments of each frame in float64, rounded once to dtype"""
    f64 = np.asarray(frames, dtype=np.float32).astype(np.float64)
    mean = f64.mean(axis=(-2, -1), keepdims=True)
    std = np.sqrt(((f64 - mean) ** 2).mean(axis=(-2, -1), keepdims=True))
    mean, std = mean.astype(dtype), np.maximum(std.astype(dtype), dtype(1e-6))
    return (np.asarray(frames, dtype=np.float32).astype(dtype) - mean) / std


def _binomial_even(p, axis):
    """[1 4 6 4 1] / 16 along axis at the even positions, replicate border: ((p[-2] + p[2]) + 4 (p[-1] + p[1]) + 6 p[0]) / 16"""
    dt = p.dtype.type
    n = p.shape[axis]
    c = np.arange(0, n, 2)
    t = lambda d: np.take(p, np.clip(c + d, 0, n - 1), axis=axis)
    s = (t(-2) + t(2)) + dt(4) * (t(-1) + t(1))
    return (s + dt(6) * t(0)) * dt(0.0625)


def downsample(p):
    """(..., h, w) -> (..., ceil(h / 2), ceil(w / 2)): the binomial along the rows (over x), then along the columns (over y)"""
    return _binomial_even(_binomial_even(p, -1), -2)


def pyramid(frames, min_size, dtype):
    levels = [normalise(frames, dtype)]
    for _ in level_sizes(frames.shape[-2], frames.shape[-1], min_size)[1:]:
        levels.append(downsample(levels[-1]))
    return levels


def bilinear(img, x, y):
    """img (P, h, w) at the positions x, y (P, H, W), clamped into the image:
    (I00 (1 - fx) + I01 fx) (1 - fy) + (I10 (1 - fx) + I11 fx) fy"""
    dt = img.dtype.type
    h, w = img.shape[-2:]
    x = np.minimum(np.maximum(x, dt(0)), dt(w - 1))
    y = np.minimum(np.maximum(y, dt(0)), dt(h - 1))
    x0 = np.floor(x).astype(np.int64)
    y0 = np.floor(y).astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    fx = x - x0.astype(img.dtype)
    fy = y - y0.astype(img.dtype)
    gx, gy = dt(1) - fx, dt(1) - fy
    k = np.arange(img.shape[0])[:, None, None]
    top = img[k, y0, x0] * gx + img[k, y0, x1] * fx
    bot = img[k, y1, x0] * gx + img[k, y1, x1] * fx
    return top * gy + bot * fy


def _grid(h, w, dtype):
    return np.arange(w, dtype=dtype)[None, None, :], np.arange(h, dtype=dtype)[None, :, None]


def upsample(uc, h, w):
    """u (P, hc, wc) -> 2 bilinear(u, x / 2, y / 2) at (P, h, w)"""
    dt = uc.dtype.type
    xs, ys = _grid(h, w, uc.dtype)
    shape = (uc.shape[0], h, w)
    return dt(2) * bilinear(uc, np.broadcast_to(xs * dt(0.5), shape), np.broadcast_to(ys * dt(0.5), shape))


def warp_terms(a, b, u, v):
    """-> bw, Ix, Iy, It of the pair (a, b) under the flow (u, v), all (P, h, w)"""
    dt = a.dtype.type
    xs, ys = _grid(a.shape[-2], a.shape[-1], a.dtype)
    bw = bilinear(b, xs + u, ys + v)
    m = np.pad((a + bw) * dt(0.5), [(0, 0), (1, 1), (1, 1)], mode='edge')
    Ix = (m[:, 1:-1, 2:] - m[:, 1:-1, :-2]) * dt(0.5)
    Iy = (m[:, 2:, 1:-1] - m[:, :-2, 1:-1]) * dt(0.5)
    return bw, Ix, Iy, bw - a


def _refresh(p):
    """the replicate border of a padded (P, h + 2, w + 2) array from its interior"""
    p[:, 0, 1:-1] = p[:, 1, 1:-1]
    p[:, -1, 1:-1] = p[:, -2, 1:-1]
    p[:, :, 0] = p[:, :, 1]
    p[:, :, -1] = p[:, :, -2]


def _average(p, c6, c12):
    """Horn-Schunck average of a padded array: ((l + r) + (t + b)) / 6 + ((tl + tr) + (bl + br)) / 12"""
    e = (p[:, 1:-1, :-2] + p[:, 1:-1, 2:]) + (p[:, :-2, 1:-1] + p[:, 2:, 1:-1])
    d = (p[:, :-2, :-2] + p[:, :-2, 2:]) + (p[:, 2:, :-2] + p[:, 2:, 2:])
    return e * c6 + d * c12


def jacobi(u, v, Ix, Iy, It, alpha, iters):
    """iters Jacobi steps from (u, v) = (u0, v0):  r = ((Ix (ub - u0) + Iy (vb - v0)) + It) / den,  u = ub - Ix r,  v = vb - Iy r"""
    dt = u.dtype.type
    a = dt(np.float32(alpha))
    den = (a * a + Ix * Ix) + Iy * Iy
    c6, c12 = dt(np.float32(1.0 / 6.0)), dt(np.float32(1.0 / 12.0))
    up = np.pad(u, [(0, 0), (1, 1), (1, 1)], mode='edge')
    vp = np.pad(v, [(0, 0), (1, 1), (1, 1)], mode='edge')
    for _ in range(iters):
        ub, vb = _average(up, c6, c12), _average(vp, c6, c12)
        r = ((Ix * (ub - u) + Iy * (vb - v)) + It) / den
        up[:, 1:-1, 1:-1] = ub - Ix * r
        vp[:, 1:-1, 1:-1] = vb - Iy * r
        _refresh(up)
        _refresh(vp)
    return up[:, 1:-1, 1:-1].copy(), vp[:, 1:-1, 1:-1].copy()


def dense_flow(frames, alpha=1.0, warps=3, iters=64, min_size=8, dtype=np.float64, debug_level=0):
    """frames (n, tl, H, W) float32 -> dict
        pyr     list over the levels k (0: finest) of (n, tl, h_k, w_k): the normalised pyramid
        levels  list over the levels k of (n, tl (tl - 1), 2, h_k, w_k): the flow when level k is left (pairs in the order of pairs())
        warp    (4, n, tl (tl - 1), h, w): bw, Ix, Iy, It of the last warp at level debug_level
        flow    (n, tl tl, 2, H, W): entry i tl + j is the flow from frame i to frame j, zeros on the diagonal"""
    frames = np.asarray(frames, dtype=np.float32)
    n, tl, H, W = frames.shape
    dtype = np.dtype(dtype).type
    pyr = pyramid(frames, min_size, dtype)
    pr = pairs(tl)
    ia = np.array([i for i, _ in pr])
    ib = np.array([j for _, j in pr])
    out = {'pyr': pyr, 'levels': [None] * len(pyr), 'warp': None}
    u = v = None
    for k in range(len(pyr) - 1, -1, -1):
        h, w = pyr[k].shape[-2:]
        a = pyr[k][:, ia].reshape(-1, h, w)
        b = pyr[k][:, ib].reshape(-1, h, w)
        if u is None:
            u, v = np.zeros_like(a), np.zeros_like(a)
        else:
            u, v = upsample(u, h, w), upsample(v, h, w)
        for s in range(warps):
            bw, Ix, Iy, It = warp_terms(a, b, u, v)
            if k == debug_level and s == warps - 1:
                out['warp'] = np.stack([bw, Ix, Iy, It]).reshape(4, n, len(pr), h, w)
            u, v = jacobi(u, v, Ix, Iy, It, alpha, iters)
        out['levels'][k] = np.stack([u, v], axis=1).reshape(n, len(pr), 2, h, w)
    flow = np.zeros((n, tl * tl, 2, H, W), dtype=dtype)
    flow[:, ia * tl + ib] = out['levels'][0]
    out['flow'] = flow
    return out


def stage_tolerance(ref32, ref64):
    """what the device may deviate from ref64 at a stage: 16 max|ref32 - ref64| + 16 2^-23 max(1, max|ref64|)"""
    r64 = np.asarray(ref64, dtype=np.float64)
    d = float(np.abs(np.asarray(ref32, dtype=np.float64) - r64).max()) if r64.size else 0.0
    return 16.0 * d + 16.0 * 2.0 ** -23 * max(1.0, float(np.abs(r64).max()) if r64.size else 0.0)
