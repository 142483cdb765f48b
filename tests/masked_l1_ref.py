"""numpy restatement of the masked multi-scale pseudo-GT term (include/dis_hip.h: dis_masked_l1_multi_fwd / _bwd) and, next to it, a
triple-loop brute force the restatement is checked against.  Terms in float32, sums in float64, as the kernels form them.

    valid(p, y, x)  target > 0 at every pixel of the (2r+1)^2 window around (y, x) inside the image, in plane p
    val_s           float32( sum over valid of float64(|o_s - t| in float32) / float64(N) ),  N = valid pixels of the call; 0 if N = 0
    grad_s          valid ? sign(o_s - t) * (gscale_s / float32(N)) : 0;                      all 0 if N = 0
"""
import numpy as np


def planes_of(a):
    """(tl, bs, 1, H, W) or (N, 1, H, W) or (planes, H, W) -> float32 (planes, H, W)"""
    a = np.asarray(a, dtype=np.float32)
    return a.reshape((-1,) + a.shape[-2:])


def valid_mask(t, r):
    """t (planes, H, W) float32 -> bool (planes, H, W): the erosion of t > 0 by a (2r+1)^2 window clipped at the image"""
    t = planes_of(t)
    with np.errstate(invalid='ignore'):
        pos = t > 0                      # (NaN > 0 is False: a hole)
    _, h, w = t.shape
    pad = np.ones((t.shape[0], h + 2 * r, w + 2 * r), dtype=bool)   # outside the image nothing invalidates
    pad[:, r:r + h, r:r + w] = pos
    v = np.ones_like(pos)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            v &= pad[:, dy:dy + h, dx:dx + w]
    return v


def masked_l1_multi(outs, t, r=0, gscales=None):
    """-> (values: list of np.float32, grads: list of float32 arrays shaped like the estimates, N: int).
    gscales: per estimate the incoming gradient of its value (default 1)."""
    shape = np.asarray(outs[0]).shape
    tp = planes_of(t)
    v = valid_mask(tp, r)
    n = int(v.sum())
    gscales = [1.0] * len(outs) if gscales is None else gscales
    vals, grads = [], []
    for o, gs in zip(outs, gscales):
        op = planes_of(o)
        with np.errstate(invalid='ignore', over='ignore'):
            d = op - tp                  # float32
            a = np.abs(d)
        if n == 0:
            vals.append(np.float32(0))
            grads.append(np.zeros(shape, dtype=np.float32))
            continue
        vals.append(np.float32(a[v].astype(np.float64).sum() / np.float64(n)))
        g = np.float32(gs) / np.float32(n)
        with np.errstate(invalid='ignore'):
            sg = np.where(d > 0, g, np.where(d < 0, -g, np.float32(0))).astype(np.float32)
        grads.append(np.where(v, sg, np.float32(0)).astype(np.float32).reshape(shape))
    return vals, grads, n


def brute_force(outs, t, r=0, gscales=None):
    """the same by loops over every pixel and every window position, sharing no code with the restatement"""
    tp = planes_of(t)
    P, H, W = tp.shape
    valid = np.zeros((P, H, W), dtype=bool)
    for p in range(P):
        for y in range(H):
            for x in range(W):
                ok = True
                for yy in range(y - r, y + r + 1):
                    for xx in range(x - r, x + r + 1):
                        if 0 <= yy < H and 0 <= xx < W and not (tp[p, yy, xx] > 0):
                            ok = False
                valid[p, y, x] = ok
    n = int(valid.sum())
    gscales = [1.0] * len(outs) if gscales is None else gscales
    vals, grads = [], []
    for o, gs in zip(outs, gscales):
        op = planes_of(o)
        total = np.float64(0)
        g = np.zeros((P, H, W), dtype=np.float32)
        for p in range(P):
            for y in range(H):
                for x in range(W):
                    if not valid[p, y, x]:
                        continue
                    d = np.float32(op[p, y, x]) - np.float32(tp[p, y, x])
                    total += np.float64(np.float32(abs(d)))
                    step = np.float32(gs) / np.float32(n)
                    g[p, y, x] = step if d > 0 else (-step if d < 0 else np.float32(0))
        vals.append(np.float32(total / np.float64(n)) if n else np.float32(0))
        grads.append(g.reshape(np.asarray(o).shape))
    return vals, grads, n


def dyadic(rng, shape):
    """multiples of 1/64 in (-256, 256): differences and their fp64 sums are exact whatever the order"""
    return (rng.randint(-256 * 64 + 1, 256 * 64, size=shape).astype(np.float32) / np.float32(64)).astype(np.float32)


def hole_layouts(planes, h, w):
    """name -> bool (planes, h, w) hole mask: the layouts the CPU and GPU tests share"""
    out = {}
    m = np.zeros((planes, h, w), dtype=bool)
    m[:, 0, 0] = m[:, 0, -1] = m[:, -1, 0] = m[:, -1, -1] = True
    out['corners'] = m
    m = np.zeros((planes, h, w), dtype=bool)
    m[0, -1, :] = True                   # must not invalidate row 0 of plane 1
    out['last_row_plane0'] = m
    m = np.zeros((planes, h, w), dtype=bool)
    m[min(1, planes - 1)] = True
    out['all_hole_plane'] = m
    out['all_holes'] = np.ones((planes, h, w), dtype=bool)
    return out


def punch(t, holes, value=0.0):
    t = np.array(t, dtype=np.float32, copy=True)
    t.reshape((-1,) + t.shape[-2:])[holes.reshape((-1,) + holes.shape[-2:])] = np.float32(value)
    return t
