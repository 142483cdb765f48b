"""Numpy restatement of the pairwise pose estimation (include/dis_hip.h, section "track poses") - and nothing else.  Parameterised by
dtype: float64 is the oracle; float32 forms every per-pixel term in float32 and adds the terms in float64, which is what csrc/pose.hip
does (the state and the solve are float64 in both).  Every per-pixel expression is written in the operand order of the header."""
import numpy as np

# the entries of J_r that are not structurally zero (the others are skipped, never multiplied)
NONZERO = ((0, 1, 2, 3, 5), (0, 1, 2, 4, 5), (0, 1, 5))
NSUMS = 30   # H_pq (p <= q, row by row): 0 .. 20; g_p: 21 .. 26; S_w: 27; S_c: 28; n: 29


def hidx(p, q):
    return p * 6 - p * (p - 1) // 2 + (q - p)


def _valid(d):
    return np.isfinite(d) & (d > 0)


def _targets(di, dj, fl, fx, fy, cx, cy, fb, dt):
    """the matched pixels of pair (i, j): P (3, m), uj, vj, ds (m) in dt, and their count"""
    H, W = di.shape
    with np.errstate(all='ignore'):
        vi, vjm = _valid(di), _valid(dj)
        u = np.broadcast_to(np.arange(W, dtype=dt)[None, :], (H, W))
        v = np.broadcast_to(np.arange(H, dtype=dt)[:, None], (H, W))
        uj, vj = u + fl[0].astype(dt), v + fl[1].astype(dt)
        ok = vi & (uj >= 0) & (uj <= dt(W - 1)) & (vj >= 0) & (vj <= dt(H - 1))
        x0 = np.minimum(np.floor(np.where(ok, uj, 0)).astype(np.int64), W - 2)
        y0 = np.minimum(np.floor(np.where(ok, vj, 0)).astype(np.int64), H - 2)
        ok = ok & vjm[y0, x0] & vjm[y0, x0 + 1] & vjm[y0 + 1, x0] & vjm[y0 + 1, x0 + 1]
    u, v, uj, vj, x0, y0 = (a[ok] for a in (u, v, uj, vj, x0, y0))
    d = di[ok].astype(dt)
    djd = dj.astype(dt)
    ax, ay = uj - x0.astype(dt), vj - y0.astype(dt)
    gx, gy = dt(1) - ax, dt(1) - ay
    ds = (djd[y0, x0] * gx + djd[y0, x0 + 1] * ax) * gy + (djd[y0 + 1, x0] * gx + djd[y0 + 1, x0 + 1] * ax) * ay
    z = fb / d
    P = [z * ((u - cx) / fx), z * ((v - cy) / fy), z]
    return P, uj, vj, ds


def _sums(R, t, P, uj, vj, ds, fx, fy, cx, cy, fb, s2, first, dt):
    """the 30 sums of one pass at the state (R, t) (float64; its rounding to dt is used): float64 (30,); and the objective that the
    pass's step descends: sum r2 in pass 0, sum r2 g afterwards (Geman-McClure's, whose weight in iterated least squares is g g)"""
    Rs, ts = R.astype(dt), t.astype(dt)
    X = [((Rs[c, 0] * P[0] + Rs[c, 1] * P[1]) + Rs[c, 2] * P[2]) + ts[c] for c in range(3)]
    used = X[2] > 0
    X0, X1, X2 = (x[used] for x in X)
    uj, vj, ds = uj[used], vj[used], ds[used]
    iz = dt(1) / X2
    px, py = X0 * iz, X1 * iz
    e = [(fx * px + cx) - uj, (fy * py + cy) - vj, fb * iz - ds]
    r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    g = dt(1) / (dt(1) + r2 / s2)
    w = np.ones_like(g) if first else g * g
    a, b, c = fx * iz, fy * iz, fb * iz
    g0, g1, g2 = -(a * px), -(b * py), -(c * iz)
    J = [{0: g0 * X1, 1: a * X2 - g0 * X0, 2: -(a * X1), 3: a, 5: g0},
         {0: g1 * X1 - b * X2, 1: -(g1 * X0), 2: b * X0, 4: b, 5: g1},
         {0: g2 * X1, 1: -(g2 * X0), 5: g2}]
    S = np.zeros(NSUMS, np.float64)
    f64sum = lambda x: float(np.sum(x.astype(np.float64)))
    for r in range(3):
        assert tuple(sorted(J[r])) == NONZERO[r]
        for p in NONZERO[r]:
            wJ = w * J[r][p]
            for q in NONZERO[r]:
                if q >= p:
                    S[hidx(p, q)] += f64sum(wJ * J[r][q])
            S[21 + p] += f64sum(wJ * e[r])
    S[27] = f64sum(w)
    S[28] = f64sum(w * r2)
    S[29] = float(X2.size)
    return S, f64sum(r2 if first else r2 * g)


def solve_step(S, R, t, damping, min_corr):
    """one Gauss-Newton step in float64 from the sums S: -> (R, t, ok).  A failed step returns the state unchanged."""
    if S[29] < min_corr:
        return R, t, False
    A = np.zeros((6, 6))
    for p in range(6):
        for q in range(p, 6):
            A[p, q] = A[q, p] = S[hidx(p, q)]
    for p in range(6):
        A[p, p] = A[p, p] + damping * A[p, p]
    L = np.zeros((6, 6))
    with np.errstate(all='ignore'):
        for c in range(6):
            s = A[c, c]
            for k in range(c):
                s = s - L[c, k] * L[c, k]
            if not (s > 0 and np.isfinite(s)):
                return R, t, False
            L[c, c] = np.sqrt(s)
            for r in range(c + 1, 6):
                s = A[r, c]
                for k in range(c):
                    s = s - L[r, k] * L[c, k]
                L[r, c] = s / L[c, c]
        y = np.zeros(6)
        for r in range(6):
            s = -S[21 + r]
            for k in range(r):
                s = s - L[r, k] * y[k]
            y[r] = s / L[r, r]
        d = np.zeros(6)
        for r in range(5, -1, -1):
            s = y[r]
            for k in range(r + 1, 6):
                s = s - L[k, r] * d[k]
            d[r] = s / L[r, r]
    om, nu = d[:3], d[3:]
    th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    if th2 < 1e-16:
        ca, cb = 1.0, 0.5
    else:
        th = np.sqrt(th2)
        ca, cb = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    Wx = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    W2 = np.outer(om, om) - th2 * np.eye(3)
    dR = np.eye(3) + ca * Wx + cb * W2
    return dR @ R, dR @ t + nu, True


def track_poses(disp, flow, K, baseline, iters=6, scale=1.0, damping=0.0, min_corr=64, dtype=np.float64):
    """disp (n, tl, H, W), flow (n, tl tl, 2, H, W) float32, K (3, 3) -> dict
        R_pair (n, tl, tl, 3, 3), t_pair (n, tl, tl, 3), stats (n, tl, tl, 4): the float64 state and statistics rounded to dtype
        state_R, state_t: the float64 state itself
        cost, n_used (n, tl, tl, iters + 1): the objective (sum r2 in pass 0, sum r2 g afterwards) and n of every pass, the closing one
        included (float64, int64)
        steps (n, tl, tl): how many steps were taken"""
    disp = np.asarray(disp, dtype=np.float32)
    flow = np.asarray(flow, dtype=np.float32)
    n, tl, H, W = disp.shape
    assert flow.shape == (n, tl * tl, 2, H, W)
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    fx, fy, cx, cy = f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2])
    fb = dt(np.float32(np.float32(K[0][0]) * np.float32(baseline)))     # the device forms fx baseline in float32 on the host
    s2 = dt(np.float32(np.float32(scale) * np.float32(scale)))
    damp = float(np.float32(damping))
    out = {'R_pair': np.zeros((n, tl, tl, 3, 3), dt), 't_pair': np.zeros((n, tl, tl, 3), dt), 'stats': np.zeros((n, tl, tl, 4), dt), 'state_R': np.zeros((n, tl, tl, 3, 3)), 'state_t': np.zeros((n, tl, tl, 3)),
           'cost': np.zeros((n, tl, tl, iters + 1)), 'n_used': np.zeros((n, tl, tl, iters + 1), np.int64),
           'steps': np.zeros((n, tl, tl), np.int64)}
    for b in range(n):
        for i in range(tl):
            for j in range(tl):
                R, t = np.eye(3), np.zeros(3)
                st = np.array([0, 0, 0, 1], np.float64)
                if i != j:
                    P, uj, vj, ds = _targets(disp[b, i], disp[b, j], flow[b, i * tl + j], fx, fy, cx, cy, fb, dt)
                    ok = True
                    with np.errstate(all='ignore'):
                        for k in range(iters + 1):
                            S, cost = _sums(R, t, P, uj, vj, ds, fx, fy, cx, cy, fb, s2, k == 0, dt)
                            out['cost'][b, i, j, k], out['n_used'][b, i, j, k] = cost, int(S[29])
                            if k < iters and ok:
                                R, t, ok = solve_step(S, R, t, damp, min_corr)
                                out['steps'][b, i, j] += ok
                    nc, sw, sc = S[29], S[27], S[28]
                    st = np.array([nc, sw / nc if nc > 0 else 0.0, np.sqrt(sc / sw) if (nc > 0 and sw > 0) else 0.0, 1.0 if ok else 0.0])
                out['state_R'][b, i, j], out['state_t'][b, i, j] = R, t
                out['R_pair'][b, i, j], out['t_pair'][b, i, j], out['stats'][b, i, j] = R, t, st
    return out


def tolerance(r32, r64):
    """what the device may deviate from r64 in a float output: 16 max|r32 - r64| + 16 2^-23 max(1, max|r64|)"""
    r64 = np.asarray(r64, dtype=np.float64)
    d = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max()) if r64.size else 0.0
    return 16.0 * d + 16.0 * 2.0 ** -23 * max(1.0, float(np.abs(r64).max()) if r64.size else 0.0)
