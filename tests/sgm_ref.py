"""Numpy restatement of the semi-global matcher (include/dis_hip.h, section "semi-global matching"): what csrc/sgm.hip must equal
bit for bit.  Written for clarity and for whole-array numpy operations, not after the kernels: the cost volume is materialised, the
paths are swept column by column (row by row for the vertical ones) over all lines at once."""
import numpy as np

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))   # (dx, dy)
_POP8 = np.array([bin(i).count('1') for i in range(256)], dtype=np.uint8)


def census(img):
    """(..., H, W) float32 -> uint64: 9 x 7 window, replicate padding, bit k (value 2^k) = k-th neighbour < centre, the 62 neighbours in
    row-major order without the centre"""
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape[-2:]
    pad = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(3, 3), (4, 4)], mode='edge')
    out = np.zeros(img.shape, dtype=np.uint64)
    k = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = pad[..., 3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
            out |= (nb < img).astype(np.uint64) << np.uint64(k)
            k += 1
    return out


def popcount64(a):
    return _POP8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(-1, dtype=np.int32)


def cost_volume(cI, cP, ndisp):
    """cI (n, H, W), cP (H, W) uint64 -> C (n, H, W, D) int32: popcount(cI(u, v) xor cP(u - d, v)), 64 where u - d < 0"""
    n, H, W = cI.shape
    C = np.full((n, H, W, ndisp), 64, dtype=np.int32)
    for d in range(min(ndisp, W)):
        C[:, :, d:, d] = popcount64(cI[:, :, d:] ^ cP[None, :, :W - d])
    return C


def _step(C, Lp, p1, p2):
    """one step of a path: C, Lp (..., D) -> L"""
    m = Lp.min(-1, keepdims=True)
    big = np.int32(1 << 20)
    lo = np.concatenate([np.full_like(Lp[..., :1], big), Lp[..., :-1]], -1) + p1
    hi = np.concatenate([Lp[..., 1:], np.full_like(Lp[..., :1], big)], -1) + p1
    return C + np.minimum(np.minimum(Lp, m + p2), np.minimum(lo, hi)) - m


def aggregate(C, p1, p2):
    """C (n, H, W, D) -> S = sum over the 8 directions of L_r, int32"""
    n, H, W, D = C.shape
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS:
        L = np.empty_like(C)
        if dx == 0:   # vertical: sweep the rows, all columns at once
            ys = range(H) if dy > 0 else range(H - 1, -1, -1)
            prev = None
            for y in ys:
                L[:, y] = C[:, y] if prev is None else _step(C[:, y], L[:, prev], p1, p2)
                prev = y
        else:         # sweep the columns; the predecessor of row y is row y - dy of the previous column
            xs = range(W) if dx > 0 else range(W - 1, -1, -1)
            prev = None
            for x in xs:
                if prev is None:
                    L[:, :, x] = C[:, :, x]
                elif dy == 0:
                    L[:, :, x] = _step(C[:, :, x], L[:, :, prev], p1, p2)
                else:
                    Lp = L[:, :, prev]                      # (n, H, D)
                    L[:, :, x] = C[:, :, x]                 # the row without a predecessor starts a path
                    if dy > 0:
                        L[:, 1:, x] = _step(C[:, 1:, x], Lp[:, :-1], p1, p2)
                    else:
                        L[:, :-1, x] = _step(C[:, :-1, x], Lp[:, 1:], p1, p2)
                prev = x
        assert L.max() <= 64 + p2
        S += L
    return S


def winner(S, uniq, lr):
    """S (n, H, W, D) -> disp float32, d0 int32, valid bool, all (n, H, W)"""
    n, H, W, D = S.shape
    S = S.astype(np.int64)
    d0 = S.argmin(-1)                                   # numpy: the first (lowest d) on ties
    s0 = np.take_along_axis(S, d0[..., None], -1)[..., 0]
    ds = np.arange(D)
    far = np.abs(ds[None, None, None, :] - d0[..., None]) > 1
    s2 = np.where(far, S, np.int64(1 << 40)).min(-1)
    # right view: dR(x, v) = argmin over d with x + d < W of S(x + d, v, d)
    SR = np.full((n, H, W, D), np.int64(1 << 40))
    for d in range(min(D, W)):
        SR[:, :, :W - d, d] = S[:, :, d:, d]
    dR = SR.argmin(-1)
    u = np.arange(W)[None, None, :]
    xr = u - d0
    ok = (d0 >= 1) & (d0 <= D - 2) & (s2 * (100 - int(uniq)) > s0 * 100) & (xr >= 0)
    dRw = np.take_along_axis(dR, np.clip(xr, 0, W - 1), -1)
    ok &= np.abs(dRw - d0) <= int(lr)
    dm, dp = np.clip(d0 - 1, 0, D - 1), np.clip(d0 + 1, 0, D - 1)
    a = np.take_along_axis(S, dm[..., None], -1)[..., 0].astype(np.float32)
    b = s0.astype(np.float32)
    c = np.take_along_axis(S, dp[..., None], -1)[..., 0].astype(np.float32)
    den = a + c - np.float32(2) * b
    with np.errstate(divide='ignore', invalid='ignore'):
        sub = d0.astype(np.float32) + (a - c) / (np.float32(2) * den)
    disp = np.where(den > 0, sub, d0.astype(np.float32)).astype(np.float32)
    disp = np.where(ok, disp, np.float32(0)).astype(np.float32)
    return disp, d0.astype(np.int32), ok


def sgm_disparity(im, pattern, ndisp=64, p1=7, p2=60, uniq=5, lr=1):
    """im (n, H, W), pattern (H, W) -> dict: disp float32, d_int int32, valid bool (n, H, W); vol int16 (n, H, W, D); census int64
    (n + 1, H, W), the pattern's last"""
    im = np.asarray(im, dtype=np.float32)
    pattern = np.asarray(pattern, dtype=np.float32)
    assert im.ndim == 3 and pattern.shape == im.shape[1:]
    assert ndisp in (64, 128, 256) and 0 < p1 < p2 <= 127 and 0 <= uniq < 100 and lr >= 0
    cI, cP = census(im), census(pattern)
    S = aggregate(cost_volume(cI, cP, ndisp), int(p1), int(p2))
    assert S.max() <= 8 * (64 + p2)
    disp, d0, ok = winner(S, uniq, lr)
    return {'disp': disp, 'd_int': d0, 'valid': ok, 'vol': S.astype(np.int16),
            'census': np.concatenate([cI, cP[None]], 0).view(np.int64)}
