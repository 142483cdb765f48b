"""Numpy restatement of the track fusion (include/dis_hip.h, section "track fusion") - and nothing else.  Parameterised by dtype: the
same code runs in float64 (the oracle) and in float32 (what the kernels' arithmetic is; the distance between the two gives the tests
their tolerance and the band inside which a decision may fall either way).  Every sum is written in an explicit operand order, which
csrc/fuse.hip follows."""
import numpy as np


def _valid(d):
    return np.isfinite(d) & (d > 0)


def _to_world(R, t, a):
    """R^T (a - t) with R (n, 3, 3), t (n, 3) broadcast over (n, H, W): component k = (R[0][k] q0 + R[1][k] q1) + R[2][k] q2"""
    q = [a[k] - t[:, k, None, None] for k in range(3)]
    return [(R[:, 0, k, None, None] * q[0] + R[:, 1, k, None, None] * q[1]) + R[:, 2, k, None, None] * q[2] for k in range(3)]


def fuse(disp, R, t, K, baseline, value=None, tol=0.01, min_views=2, dtype=np.float64):
    """disp (n, tl, H, W) float32, R (n, tl, 3, 3), t (n, tl, 3), K (3, 3) -> dict
        valid, keep (n, tl, H, W) bool; views, seen (n, tl, H, W) uint8; resid (n, tl, H, W); point, normal (n, tl, 3, H, W)
        seen_ij, cons_ij (n, tl, tl, H, W) bool; rel, uj, vj, zj (n, tl, tl, H, W): pair (i, j) at [:, i, j]; zj is X_j.z
        ndot (n, tl, H, W): n . P of the unflipped unit normal (0 where the normal is zero)
        xyz, normal_packed (m, 3), value (m), src (m) int32, count (n) int32: the packed list"""
    disp = np.asarray(disp, dtype=np.float32)
    n, tl, H, W = disp.shape
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    R = np.asarray(R, dtype=np.float32).astype(dt)
    t = np.asarray(t, dtype=np.float32).astype(dt)
    fx, fy, cx, cy = f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2])
    fb = fx * f32(baseline)
    tolv = f32(tol)
    valid = _valid(disp)
    with np.errstate(all='ignore'):
        d = np.where(valid, disp, np.float32(1)).astype(dt)
        z = fb / d                                                     # depth of every frame (1-disparity where invalid, never used)
        rx = ((np.arange(W, dtype=dt) - cx) / fx)[None, None, None, :]
        ry = ((np.arange(H, dtype=dt) - cy) / fy)[None, None, :, None]
        P = [z * rx, z * ry, z]                                        # (n, tl, H, W) each
        shape5 = (n, tl, tl, H, W)
        seen_ij, cons_ij = np.zeros(shape5, bool), np.zeros(shape5, bool)
        rel, uj_, vj_, zj_ = (np.zeros(shape5, dt) for _ in range(4))
        views = np.zeros((n, tl, H, W), np.int64)
        seen = np.zeros((n, tl, H, W), np.int64)
        resid = np.zeros((n, tl, H, W), dt)
        point = np.zeros((n, tl, 3, H, W), dt)
        normal = np.zeros((n, tl, 3, H, W), dt)
        ndot = np.zeros((n, tl, H, W), dt)
        lower = np.zeros((n, tl, H, W), bool)
        k_ = np.arange(n)[:, None, None]
        for i in range(tl):
            Pi = [P[c][:, i] for c in range(3)]
            Xw = _to_world(R[:, i], t[:, i], Pi)
            acc = [x.copy() for x in Xw]
            rsum = np.zeros((n, H, W), dt)
            vi = valid[:, i]
            views[:, i] = vi
            for j in range(tl):
                if j == i:
                    continue
                Rj, tj = R[:, j], t[:, j]
                Xj = [((Rj[:, c, 0, None, None] * Xw[0] + Rj[:, c, 1, None, None] * Xw[1]) + Rj[:, c, 2, None, None] * Xw[2])
                      + tj[:, c, None, None] for c in range(3)]
                uj = (fx * Xj[0]) / Xj[2] + cx
                vj = (fy * Xj[1]) / Xj[2] + cy
                ok = vi & (Xj[2] > 0) & (uj >= 0) & (uj <= dt(W - 1)) & (vj >= 0) & (vj <= dt(H - 1))
                x0 = np.minimum(np.floor(np.where(ok, uj, 0)).astype(np.int64), W - 2)
                y0 = np.minimum(np.floor(np.where(ok, vj, 0)).astype(np.int64), H - 2)
                vjm, zjm = valid[:, j], z[:, j]
                ok = ok & vjm[k_, y0, x0] & vjm[k_, y0, x0 + 1] & vjm[k_, y0 + 1, x0] & vjm[k_, y0 + 1, x0 + 1]
                ax, ay = uj - x0.astype(dt), vj - y0.astype(dt)
                gx, gy = dt(1) - ax, dt(1) - ay
                zs = (zjm[k_, y0, x0] * gx + zjm[k_, y0, x0 + 1] * ax) * gy + (zjm[k_, y0 + 1, x0] * gx + zjm[k_, y0 + 1, x0 + 1] * ax) * ay
                r = np.abs(zs - Xj[2]) / Xj[2]
                cons = ok & (np.where(ok, r, np.inf) <= tolv)
                s = zs / Xj[2]
                Sw = _to_world(Rj, tj, [Xj[0] * s, Xj[1] * s, Xj[2] * s])
                for c in range(3):
                    acc[c] = np.where(cons, acc[c] + Sw[c], acc[c])
                rsum = np.where(ok, rsum + r, rsum)
                seen[:, i] += ok
                views[:, i] += cons
                if j < i:
                    lower[:, i] |= cons
                seen_ij[:, i, j], cons_ij[:, i, j] = ok, cons
                rel[:, i, j] = np.where(ok, r, 0)
                uj_[:, i, j], vj_[:, i, j], zj_[:, i, j] = uj, vj, Xj[2]
            resid[:, i] = np.where(seen[:, i] > 0, rsum / np.maximum(seen[:, i], 1).astype(dt), 0)
            for c in range(3):
                point[:, i, c] = np.where(vi, acc[c] / np.maximum(views[:, i], 1).astype(dt), 0)
            # the normal: central differences of P, interior pixels with four valid neighbours
            a = [Pi[c][:, 1:-1, 2:] - Pi[c][:, 1:-1, :-2] for c in range(3)]
            b = [Pi[c][:, 2:, 1:-1] - Pi[c][:, :-2, 1:-1] for c in range(3)]
            m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            okn = (vi[:, 1:-1, 1:-1] & vi[:, 1:-1, 2:] & vi[:, 1:-1, :-2] & vi[:, 2:, 1:-1] & vi[:, :-2, 1:-1] & (ln > 0) & np.isfinite(ln))
            lns = np.where(okn, ln, 1)
            m = [np.where(okn, mc / lns, 0) for mc in m]
            dot = (m[0] * Pi[0][:, 1:-1, 1:-1] + m[1] * Pi[1][:, 1:-1, 1:-1]) + m[2] * Pi[2][:, 1:-1, 1:-1]
            m = [np.where(dot > 0, -mc, mc) for mc in m]
            Ri = R[:, i]
            for c in range(3):
                normal[:, i, c, 1:-1, 1:-1] = np.where(
                    okn, (Ri[:, 0, c, None, None] * m[0] + Ri[:, 1, c, None, None] * m[1]) + Ri[:, 2, c, None, None] * m[2], 0)
            ndot[:, i, 1:-1, 1:-1] = dot
    keep = valid & (views >= int(min_views)) & ~lower
    out = {'valid': valid, 'keep': keep, 'views': views.astype(np.uint8), 'seen': seen.astype(np.uint8), 'resid': resid, 'point': point,
           'normal': normal, 'seen_ij': seen_ij, 'cons_ij': cons_ij, 'rel': rel, 'uj': uj_, 'vj': vj_, 'zj': zj_, 'ndot': ndot}
    src = np.flatnonzero(keep.reshape(-1))
    bi, v, u = src // (H * W), (src // W) % H, src % W
    out['src'] = src.astype(np.int32)
    out['xyz'] = point.reshape(n * tl, 3, H, W)[bi, :, v, u]
    out['normal_packed'] = normal.reshape(n * tl, 3, H, W)[bi, :, v, u]
    val = np.zeros((n, tl, H, W), np.float32) if value is None else np.asarray(value, dtype=np.float32).reshape(n, tl, H, W)
    out['value'] = val.reshape(-1)[src]
    out['count'] = keep.reshape(n, -1).sum(1).astype(np.int32)
    return out


def tolerance(r32, r64):
    """what the device may deviate from r64 in a float output: 16 max|r32 - r64| + 16 2^-23 max(1, max|r64|)"""
    r64 = np.asarray(r64, dtype=np.float64)
    d = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max()) if r64.size else 0.0
    return 16.0 * d + 16.0 * 2.0 ** -23 * max(1.0, float(np.abs(r64).max()) if r64.size else 0.0)


def exempt(r32, r64, tol):
    """-> (pixels (n, tl, H, W) bool, pairs (n, tl, tl, H, W) bool): where float32 may legitimately decide differently from float64.
    A pair (i, j) of a valid pixel is exempt when
      - it is seen in float64 and |rel64 - tol| lies within the band 16 max|rel32 - rel64| + 16 2^-23 (the maximum over the pairs seen
        in both dtypes);
      - or its projected position, where X_j.z > 0, lies within the band 16 max|pos32 - pos64| + 16 2^-23 max(1, max|pos64|) (over the
        pairs seen in both) of an image edge, or of an integer cell boundary while a hole of frame j lies within two pixels of it;
      - or its `seen` flag differs between the two dtypes.
    A pixel is exempt when one of its pairs is, or when the sign of its normal hangs on roundoff: |n . P| within the band
    16 max|ndot32 - ndot64| + 16 2^-23 max(1, max|ndot64|)."""
    valid = r64['valid']
    n, tl, H, W = valid.shape
    both = r32['seen_ij'] & r64['seen_ij']
    eps = 16.0 * 2.0 ** -23
    rel32, rel64 = r32['rel'].astype(np.float64), r64['rel']
    band_r = (16.0 * float(np.abs(rel32 - rel64)[both].max()) if both.any() else 0.0) + eps
    pairs = r32['seen_ij'] != r64['seen_ij']
    pairs |= r64['seen_ij'] & (np.abs(rel64 - np.float64(np.float32(tol))) <= band_r)
    band_p = eps
    if both.any():
        dp = max(float(np.abs(r32[k].astype(np.float64) - r64[k])[both].max()) for k in ('uj', 'vj'))
        mp = max(float(np.abs(r64[k][both]).max()) for k in ('uj', 'vj'))
        band_p = 16.0 * dp + eps * max(1.0, mp)
    with np.errstate(all='ignore'):
        front = valid[:, :, None] & (r64['zj'] > 0) & np.isfinite(r64['uj']) & np.isfinite(r64['vj'])
        for i in range(tl):
            front[:, i, i] = False
        uj, vj = np.where(front, r64['uj'], 0.0), np.where(front, r64['vj'], 0.0)
        edge = (np.minimum(np.abs(uj), np.abs(uj - (W - 1))) <= band_p) | (np.minimum(np.abs(vj), np.abs(vj - (H - 1))) <= band_p)
        ru, rv = np.rint(uj), np.rint(vj)
        cell = (np.abs(uj - ru) <= band_p) | (np.abs(vj - rv) <= band_p)
        # holes of frame j within two pixels (5 x 5 dilation of the invalid mask)
        hole = ~valid
        pad = np.pad(hole, [(0, 0), (0, 0), (2, 2), (2, 2)], mode='constant')
        near = np.zeros_like(hole)
        for dy in range(5):
            for dx in range(5):
                near |= pad[:, :, dy:dy + H, dx:dx + W]
        xi = np.clip(ru, 0, W - 1).astype(np.int64)
        yi = np.clip(rv, 0, H - 1).astype(np.int64)
        inside = (uj >= -1) & (uj <= W) & (vj >= -1) & (vj <= H)
        k_ = np.arange(n)[:, None, None]
        for i in range(tl):
            for j in range(tl):
                if j != i:
                    nh = near[:, j][k_, yi[:, i, j], xi[:, i, j]]
                    pairs[:, i, j] |= front[:, i, j] & (edge[:, i, j] | (cell[:, i, j] & nh & inside[:, i, j]))
    pixels = pairs.any(axis=2)
    d32, d64 = r32['ndot'].astype(np.float64), r64['ndot']
    band_n = 16.0 * float(np.abs(d32 - d64).max()) + eps * max(1.0, float(np.abs(d64).max()))
    zero32 = ~np.any(r32['normal'] != 0, axis=2)
    zero64 = ~np.any(r64['normal'] != 0, axis=2)
    pixels = pixels | (zero32 != zero64) | (~zero64 & (np.abs(d64) <= band_n))
    return pixels, pairs
