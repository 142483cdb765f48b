"""Numpy restatement of the disparity alignment and of the rigid flow (include/dis_hip.h, section "disparity alignment") - and nothing
else.  Parameterised by dtype: float64 is the oracle; float32 forms every per-pixel term in float32 and adds the terms in float64, which
is what csrc/disp_align.hip does (the state and the solve are float64 in both: pose_ref.solve_step).  Every per-pixel expression is
written in the operand order of the header."""
import numpy as np

from tests.pose_ref import NSUMS, hidx, solve_step, tolerance   # noqa: F401  (tolerance: re-exported for the tests)

DEFAULT_ITERS = (10, 6, 4, 4, 4, 4)   # finest first
MAX_LEVELS = 6
NUDGE = 2.0 ** -6                     # the cell of a target is floor(u' + NUDGE): the identity puts every target on an integer
MARGIN = 2.0 ** -18                   # a skip test nearer than this (relative) to its threshold makes the pixel borderline


def default_levels(h, w):
    """halve while the next level keeps min(h, w) >= 24"""
    L = 1
    while L < MAX_LEVELS and min(h >> L, w >> L) >= 24:
        L += 1
    return L


def level_sizes(h, w, levels):
    return [(h >> l, w >> l) for l in range(levels)]


def level_cameras(K, levels):
    """[(fx, fy, cx, cy)] per level, formed in float32 as the host code does: fx_l = fx_{l-1} / 2, cx_l = (cx_{l-1} - 0.5) / 2"""
    f = np.float32
    c = [(f(K[0][0]), f(K[1][1]), f(K[0][2]), f(K[1][2]))]
    for _ in range(1, levels):
        fx, fy, cx, cy = c[-1]
        c.append((fx / f(2), fy / f(2), (cx - f(0.5)) / f(2), (cy - f(0.5)) / f(2)))
    return c


def _valid(d):
    with np.errstate(invalid='ignore'):
        return np.isfinite(d) & (d > 0)


def downsample(p, dt):
    """(..., h, w) -> (..., h // 2, w // 2): the mean of the valid disparities of a 2 x 2 block that are >= 0.9 x the block's largest,
    added in the order 00, 01, 10, 11; 0 without a valid one"""
    h2, w2 = p.shape[-2] // 2, p.shape[-1] // 2
    a = [p[..., dy:2 * h2:2, dx:2 * w2:2] for dy in (0, 1) for dx in (0, 1)]
    ok = [_valid(x) for x in a]
    with np.errstate(all='ignore'):
        m = np.zeros(a[0].shape, dt)
        for x, o in zip(a, ok):
            m = np.where(o & (x > m), x, m)
        thr = dt(np.float32(0.9)) * m
        s, c = np.zeros(a[0].shape, dt), np.zeros(a[0].shape, dt)
        for x, o in zip(a, ok):
            k = o & (x >= thr)
            s = np.where(k, s + x, s)
            c = np.where(k, c + dt(1), c)
        return np.where(c > 0, s / np.where(c > 0, c, dt(1)), dt(0)).astype(dt)


def pyramid(disp, levels, dt):
    """disp (n, tl, H, W) float32 -> list over the levels (0: the input, in dt)"""
    pyr = [np.asarray(disp, dtype=np.float32).astype(dt)]
    for _ in range(1, levels):
        pyr.append(downsample(pyr[-1], dt))
    return pyr


def target_maps(p, jump, dt):
    """(..., h, w) -> (..., h, w, 4) in dt: D, Dx, Dy, good (1 / 0); zeros where not good"""
    v = _valid(p)
    out = np.zeros(p.shape + (4,), dt)
    c = p[..., 1:-1, 1:-1]
    with np.errstate(all='ignore'):
        Dx = dt(0.5) * (p[..., 1:-1, 2:] - p[..., 1:-1, :-2])
        Dy = dt(0.5) * (p[..., 2:, 1:-1] - p[..., :-2, 1:-1])
        lim = jump * c
        good = (v[..., 1:-1, 1:-1] & v[..., 1:-1, 2:] & v[..., 1:-1, :-2] & v[..., 2:, 1:-1] & v[..., :-2, 1:-1]
                & (np.abs(Dx) < lim) & (np.abs(Dy) < lim))
    for k, a in enumerate((c, Dx, Dy, np.ones_like(c))):
        out[..., 1:-1, 1:-1, k] = np.where(good, a, dt(0))
    return out


def _pass(di, mj, cam, fb, R, t, unit, s2, jump2, dt, margins):
    """the 30 sums of one pass of pair (i, j) at a level: di (h, w) frame i's disparities, mj (h, w, 4) frame j's target maps, at the
    state (R, t) (float64; its rounding to dt is used) -> (S float64 (30,), the number of borderline pixels)"""
    fx, fy, cx, cy = (dt(x) for x in cam)
    h, w = di.shape
    Rs, ts = R.astype(dt), t.astype(dt)
    with np.errstate(all='ignore'):
        ok = _valid(di)
        v, u = (a[ok] for a in np.meshgrid(np.arange(h), np.arange(w), indexing='ij'))
        d = di[ok]
        z = fb / d
        P = [z * ((u.astype(dt) - cx) / fx), z * ((v.astype(dt) - cy) / fy), z]
        Y = [((Rs[c, 0] * P[0] + Rs[c, 1] * P[1]) + Rs[c, 2] * P[2]) + ts[c] for c in range(3)]
        front = Y[2] > 0
        iz = dt(1) / Y[2]
        px, py = Y[0] * iz, Y[1] * iz
        up, vp = fx * px + cx, fy * py + cy
        us, vs = up + dt(NUDGE), vp + dt(NUDGE)
        inside = front & (us >= 0) & (us < dt(w - 1)) & (vs >= 0) & (vs < dt(h - 1))
        x0 = np.where(inside, np.floor(us), 0).astype(np.int64)
        y0 = np.where(inside, np.floor(vs), 0).astype(np.int64)
        cell_good = lambda xx, yy: ((mj[yy, xx, 3] != 0) & (mj[yy, xx + 1, 3] != 0) & (mj[yy + 1, xx, 3] != 0) & (mj[yy + 1, xx + 1, 3] != 0))
        tap = inside & cell_good(x0, y0)
        ax, ay = up - x0.astype(dt), vp - y0.astype(dt)
        gx, gy = dt(1) - ax, dt(1) - ay
        bil = lambda k: (mj[y0, x0, k] * gx + mj[y0, x0 + 1, k] * ax) * gy + (mj[y0 + 1, x0, k] * gx + mj[y0 + 1, x0 + 1, k] * ax) * ay
        D, Gx, Gy = bil(0), bil(1), bil(2)
        pred = fb * iz
        e = D - pred
        lim = jump2 * pred
        used = tap & (np.abs(e) < lim)
        border = 0
        if margins:
            m = dt(MARGIN)
            zs = (np.abs(Rs[2, 0] * P[0]) + np.abs(Rs[2, 1] * P[1])) + (np.abs(Rs[2, 2] * P[2]) + np.abs(ts[2]))
            near = np.abs(Y[2]) < m * zs
            near |= front & ((np.abs(us) < m * w) | (np.abs(us - dt(w - 1)) < m * w) | (np.abs(vs) < m * h) | (np.abs(vs - dt(h - 1)) < m * h))
            # a cell boundary counts only where the cell on its other side is good and this one is not, or the reverse
            rx, ry = np.rint(np.where(inside, us, 0)), np.rint(np.where(inside, vs, 0))
            ox = np.clip(np.where(rx > x0, x0 + 1, x0 - 1), 0, w - 2)
            oy = np.clip(np.where(ry > y0, y0 + 1, y0 - 1), 0, h - 2)
            near |= inside & (np.abs(us - rx) < m * w) & (cell_good(ox, y0) != cell_good(x0, y0))
            near |= inside & (np.abs(vs - ry) < m * h) & (cell_good(x0, oy) != cell_good(x0, y0))
            near |= tap & (np.abs(np.abs(e) - lim) < m * pred)
            border = int(near.sum())
        Y0, Y1, Y2, iz, Gx, Gy, pred, e = (a[used] for a in (Y[0], Y[1], Y[2], iz, Gx, Gy, pred, e))
        g0, g1 = Gx * (fx * iz), Gy * (fy * iz)
        g2 = pred * iz - (g0 * Y0 + g1 * Y1) * iz
        J = [Y1 * g2 - Y2 * g1, Y2 * g0 - Y0 * g2, Y0 * g1 - Y1 * g0, g0, g1, g2]
        e2 = e * e
        q = dt(1) / (dt(1) + e2 / s2)
        wgt = np.ones_like(q) if unit else q * q
        S = np.zeros(NSUMS, np.float64)
        f64sum = lambda x: float(np.sum(x.astype(np.float64)))
        for a in range(6):
            wJ = wgt * J[a]
            for b in range(a, 6):
                S[hidx(a, b)] = f64sum(wJ * J[b])
            S[21 + a] = f64sum(wJ * e)
        S[27], S[28], S[29] = f64sum(wgt), f64sum(wgt * e2), float(e.size)
    return S, border


def schedule(levels, iters):
    """[(level, unit weight)] of every pass, the closing one included: the coarsest level first"""
    out = []
    for l in range(levels - 1, -1, -1):
        out += [(l, l == levels - 1 and s == 0) for s in range(int(iters[l]))]
    return out + [(0, False)]


def align_poses(disp, K, baseline, levels=None, iters=None, scale=0.3, damping=0.0, min_corr=64, jump=0.15, dtype=np.float64, margins=True):
    """disp (n, tl, H, W) float32, K (3, 3) -> dict
        R_pair (n, tl, tl, 3, 3), t_pair (n, tl, tl, 3), stats (n, tl, tl, 4): the float64 state and statistics rounded to dtype
        state_R, state_t: the float64 state itself
        sums (passes, n, tl, tl, 30) float64, n_used, borderline (n, tl, tl, passes) int64: of every pass, the closing one included
        pyr: list over the levels of (n, tl, h_l, w_l); maps: list over the levels of (n, tl, h_l, w_l, 4); sizes, cameras"""
    disp = np.asarray(disp, dtype=np.float32)
    n, tl, H, W = disp.shape
    dt = np.dtype(dtype).type
    L = default_levels(H, W) if levels is None else int(levels)
    iters = tuple(DEFAULT_ITERS[:L] if iters is None else iters)
    assert len(iters) == L
    cams = level_cameras(K, L)
    fb = dt(np.float32(np.float32(K[0][0]) * np.float32(baseline)))     # the device forms fx baseline in float32 on the host
    s2 = dt(np.float32(np.float32(scale) * np.float32(scale)))
    jmp, jump2 = dt(np.float32(jump)), dt(np.float32(np.float32(2) * np.float32(jump)))
    damp = float(np.float32(damping))
    pyr = pyramid(disp, L, dt)
    maps = [target_maps(p, jmp, dt) for p in pyr]
    sched = schedule(L, iters)
    out = {'R_pair': np.zeros((n, tl, tl, 3, 3), dt), 't_pair': np.zeros((n, tl, tl, 3), dt), 'stats': np.zeros((n, tl, tl, 4), dt),
           'state_R': np.zeros((n, tl, tl, 3, 3)), 'state_t': np.zeros((n, tl, tl, 3)), 'sums': np.zeros((len(sched), n, tl, tl, NSUMS)),
           'n_used': np.zeros((n, tl, tl, len(sched)), np.int64), 'borderline': np.zeros((n, tl, tl, len(sched)), np.int64),
           'pyr': pyr, 'maps': maps, 'sizes': level_sizes(H, W, L), 'cameras': cams, 'levels': L, 'iters': iters}
    for b in range(n):
        for i in range(tl):
            for j in range(tl):
                R, t = np.eye(3), np.zeros(3)
                st = np.array([0, 0, 0, 1], np.float64)
                if i != j:
                    ok = True
                    for k, (l, unit) in enumerate(sched):
                        S, border = _pass(pyr[l][b, i], maps[l][b, j], cams[l], fb, R, t, unit, s2, jump2, dt, margins)
                        out['sums'][k, b, i, j], out['n_used'][b, i, j, k], out['borderline'][b, i, j, k] = S, int(S[29]), border
                        if k < len(sched) - 1 and ok:
                            R, t, ok = solve_step(S, R, t, damp, min_corr)
                    nc, sw, sc = S[29], S[27], S[28]
                    st = np.array([nc, sw / nc if nc > 0 else 0.0, np.sqrt(sc / sw) if (nc > 0 and sw > 0) else 0.0, 1.0 if ok else 0.0])
                out['state_R'][b, i, j], out['state_t'][b, i, j] = R, t
                out['R_pair'][b, i, j], out['t_pair'][b, i, j], out['stats'][b, i, j] = R, t, st
    return out


def rigid_flow(disp, R, t, K, baseline, tol=0.01, dtype=np.float64):
    """disp (n, tl, H, W), R (n, tl, 3, 3), t (n, tl, 3) float32 (X_c = R X_w + t) -> flow (n, tl tl, 2, H, W) in dtype, visible
    (n, tl tl, H, W) uint8 and `borderline` (n, tl tl, H, W) bool: a test of `visible` is nearer than MARGIN to its threshold"""
    disp = np.asarray(disp, dtype=np.float32)
    n, tl, H, W = disp.shape
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    fx, fy, cx, cy = f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2])
    fb = dt(np.float32(np.float32(K[0][0]) * np.float32(baseline)))
    tol = f32(tol)
    R, t = np.asarray(R, dtype=np.float32).astype(dt), np.asarray(t, dtype=np.float32).astype(dt)
    flow = np.zeros((n, tl * tl, 2, H, W), dt)
    vis = np.zeros((n, tl * tl, H, W), np.uint8)
    border = np.zeros((n, tl * tl, H, W), bool)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    uf, vf = u.astype(dt), v.astype(dt)
    for b in range(n):
        for i in range(tl):
            d = disp[b, i].astype(dt)
            ok = _valid(d)
            with np.errstate(all='ignore'):
                z = fb / d
                P = [z * ((uf - cx) / fx), z * ((vf - cy) / fy), z]
                q = [P[k] - t[b, i, k] for k in range(3)]
                X = [(R[b, i, 0, k] * q[0] + R[b, i, 1, k] * q[1]) + R[b, i, 2, k] * q[2] for k in range(3)]
                for j in range(tl):
                    if j == i:
                        continue
                    Y = [((R[b, j, k, 0] * X[0] + R[b, j, k, 1] * X[1]) + R[b, j, k, 2] * X[2]) + t[b, j, k] for k in range(3)]
                    use = ok & (Y[2] > 0)
                    uj, vj = (fx * Y[0]) / Y[2] + cx, (fy * Y[1]) / Y[2] + cy
                    flow[b, i * tl + j, 0] = np.where(use, uj - uf, dt(0))
                    flow[b, i * tl + j, 1] = np.where(use, vj - vf, dt(0))
                    ur, vr = uj + dt(0.5), vj + dt(0.5)
                    inside = use & (ur >= 0) & (ur < dt(W)) & (vr >= 0) & (vr < dt(H))
                    xr = np.where(inside, np.floor(ur), 0).astype(np.int64)
                    yr = np.where(inside, np.floor(vr), 0).astype(np.int64)
                    dj = disp[b, j].astype(dt)[yr, xr]
                    pred = fb / Y[2]
                    lim = tol * pred
                    vis[b, i * tl + j] = inside & _valid(dj) & (np.abs(dj - pred) <= lim)
                    m = dt(MARGIN)
                    border[b, i * tl + j] = use & ((np.abs(ur - np.rint(ur)) < m * W) | (np.abs(vr - np.rint(vr)) < m * H)
                                                   | (inside & (np.abs(np.abs(dj - pred) - lim) < m * pred)))
    return flow, vis, border
