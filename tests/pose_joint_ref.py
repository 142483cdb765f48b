"""Numpy restatement of the joint pose refinement (include/dis_hip.h, section "track poses", dis_refine_track_poses) - and nothing else.
The per-pixel part is tests/pose_ref.py's own (_targets, _sums): this file adds the composition of a pair from two frames, the
assembly of the 6 (tl - 1) system through the adjoint of every pair, its solve and the statistics, each written as loops in the
operand order of csrc/pose.hip.  Parameterised by dtype like pose_ref: float64 is the oracle, float32 forms the per-pixel terms in
float32; the state, the assembly and the solve are float64 in both."""
import numpy as np

from tests.pose_ref import _sums, _targets, hidx


def compose(R, t, i, j):
    """the pair (i, j) of the frames R (tl, 3, 3), t (tl, 3), float64: R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i"""
    Rij, tij = np.zeros((3, 3)), np.zeros(3)
    for r in range(3):
        for c in range(3):
            Rij[r, c] = (R[j][r, 0] * R[i][c, 0] + R[j][r, 1] * R[i][c, 1]) + R[j][r, 2] * R[i][c, 2]
    for r in range(3):
        tij[r] = t[j][r] - ((Rij[r, 0] * t[i][0] + Rij[r, 1] * t[i][1]) + Rij[r, 2] * t[i][2])
    return Rij, tij


def adjoint(Rij, tij):
    """Ad = [[R, 0], [[t]x R, R]] on (omega, nu)"""
    Ad = np.zeros((6, 6))
    for r in range(3):
        r1, r2 = (r + 1) % 3, (r + 2) % 3
        for c in range(3):
            Ad[r, c] = Ad[3 + r, 3 + c] = Rij[r, c]
            Ad[3 + r, c] = tij[r1] * Rij[r2, c] - tij[r2] * Rij[r1, c]
    return Ad


def pair_blocks(S, Ad):
    """H (6, 6, symmetric), g (6) of the sums S; M = H Ad, N = Ad^T M, q = Ad^T g: every element the sum over k = 0 .. 5 in this order,
    from the first product"""
    H = np.zeros((6, 6))
    for p in range(6):
        for q in range(p, 6):
            H[p, q] = H[q, p] = S[hidx(p, q)]
    g = S[21:27].copy()
    M = H[:, 0:1] * Ad[0:1, :]
    for k in range(1, 6):
        M = M + H[:, k:k + 1] * Ad[k:k + 1, :]
    N_ = Ad[0:1, :].T * M[0:1, :]
    q = Ad[0, :] * g[0]
    for k in range(1, 6):
        N_ = N_ + Ad[k:k + 1, :].T * M[k:k + 1, :]
        q = q + Ad[k, :] * g[k]
    return H, g, M, N_, q


def assemble(tl, sums, ads, contrib):
    """sums, ads: dicts over the pairs (i, j); contrib: the pairs that contribute -> A (m, m), b (m), m = 6 (tl - 1): the pairs added in
    ascending (i, j), the rows and columns of frame 0 dropped"""
    m = 6 * (tl - 1)
    A, b = np.zeros((m, m)), np.zeros(m)
    for i in range(tl):
        for j in range(tl):
            if (i, j) not in contrib:
                continue
            H, g, M, N_, q = pair_blocks(sums[(i, j)], ads[(i, j)])
            si, sj = slice(6 * (i - 1), 6 * i), slice(6 * (j - 1), 6 * j)
            if j > 0:
                A[sj, sj] = A[sj, sj] + H
                b[sj] = b[sj] + g
            if i > 0:
                A[si, si] = A[si, si] + N_
                b[si] = b[si] - q
            if i > 0 and j > 0:
                A[sj, si] = A[sj, si] - M
                A[si, sj] = A[si, sj] - M.T
    return A, b


def solve(A, b, damping):
    """-(A + damping diag(A))^-1 b by Cholesky, or None at a pivot that is not > 0 or not finite.  Forward substitution with k
    ascending, backward with k descending (the device updates the rows below / above a solved unknown together); an unknown is its
    row's sum times 1 / L_kk, the reciprocal formed once per column."""
    m = len(b)
    A = A.copy()
    for p in range(m):
        A[p, p] = A[p, p] + damping * A[p, p]
    L = np.zeros((m, m))
    with np.errstate(all='ignore'):
        for c in range(m):
            s = A[c, c]
            for k in range(c):
                s = s - L[c, k] * L[c, k]
            if not (s > 0 and np.isfinite(s)):
                return None
            L[c, c] = np.sqrt(s)
            for r in range(c + 1, m):
                s = A[r, c]
                for k in range(c):
                    s = s - L[r, k] * L[c, k]
                L[r, c] = s / L[c, c]
        linv = np.array([1.0 / L[c, c] for c in range(m)])
        y = np.zeros(m)
        for r in range(m):
            s = -b[r]
            for k in range(r):
                s = s - L[r, k] * y[k]
            y[r] = s * linv[r]
        d = np.zeros(m)
        for r in range(m - 1, -1, -1):
            s = y[r]
            for k in range(m - 1, r, -1):
                s = s - L[k, r] * d[k]
            d[r] = s * linv[r]
    return d


def exp_update(d, R, t):
    """the exponential-map update of pose_ref.solve_step: R <- dR R, t <- dR t + nu"""
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
    return dR @ R, dR @ t + nu


class Track:
    """one track's fixed per-pixel data (the targets of every used pair) and the camera, in dtype dt"""

    def __init__(self, disp, flow, K, baseline, scale, use, dt):
        tl = disp.shape[0]
        f32 = lambda x: dt(np.float32(x))
        self.dt, self.tl = dt, tl
        self.cam = (f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2]), dt(np.float32(np.float32(K[0][0]) * np.float32(baseline))))
        self.s2 = dt(np.float32(np.float32(scale) * np.float32(scale)))
        self.pairs = [(i, j) for i in range(tl) for j in range(tl) if i != j and use[i, j]]
        self.targets = {(i, j): _targets(disp[i], disp[j], flow[i * tl + j], *self.cam, dt) for (i, j) in self.pairs}

    def pass_(self, R, t, min_corr):
        """one pass at the frames' state (float64): -> sums, adjoints, the contributing pairs, the objective sum r2 g over them"""
        sums, ads, contrib, cost = {}, {}, [], 0.0
        with np.errstate(all='ignore'):
            for (i, j) in self.pairs:
                Rij, tij = compose(R, t, i, j)
                S, c = _sums(Rij, tij, *self.targets[(i, j)], *self.cam, self.s2, False, self.dt)
                sums[(i, j)], ads[(i, j)] = S, adjoint(Rij, tij)
                if S[29] >= min_corr:
                    contrib.append((i, j))
                    cost += c
        return sums, ads, contrib, cost


def refine_track_poses(disp, flow, K, baseline, R_init, t_init, pair_use=None, iters=6, scale=1.0, damping=0.0, min_corr=64,
                       dtype=np.float64):
    """disp (n, tl, H, W), flow (n, tl tl, 2, H, W), R_init (n, tl, 3, 3), t_init (n, tl, 3) float32, pair_use (n, tl, tl) or None -> dict
        R (n, tl, 3, 3), t (n, tl, 3), pair_stats (n, tl, tl, 4), track_stats (n, 4): the float64 values rounded to dtype
        state_R, state_t: the float64 state itself
        cost (n, iters + 1): the objective sum r2 g over the contributing pairs of every pass; steps (n): how many steps were taken"""
    disp, flow = np.asarray(disp, dtype=np.float32), np.asarray(flow, dtype=np.float32)
    n, tl, H, W = disp.shape
    assert flow.shape == (n, tl * tl, 2, H, W)
    dt = np.dtype(dtype).type
    damp = float(np.float32(damping))
    out = {'R': np.zeros((n, tl, 3, 3), dt), 't': np.zeros((n, tl, 3), dt), 'pair_stats': np.zeros((n, tl, tl, 4), dt),
           'track_stats': np.zeros((n, 4), dt), 'state_R': np.zeros((n, tl, 3, 3)), 'state_t': np.zeros((n, tl, 3)),
           'cost': np.zeros((n, iters + 1)), 'steps': np.zeros(n, np.int64)}
    for b in range(n):
        use = np.ones((tl, tl), bool) if pair_use is None else np.asarray(pair_use[b]) != 0
        trk = Track(disp[b], flow[b], K, baseline, scale, use, dt)
        R = np.asarray(R_init[b], dtype=np.float32).astype(np.float64)
        t = np.asarray(t_init[b], dtype=np.float32).astype(np.float64)
        ok = True
        for k in range(iters + 1):
            sums, ads, contrib, cost = trk.pass_(R, t, min_corr)
            out['cost'][b, k] = cost
            if k < iters and ok:
                A, bv = assemble(tl, sums, ads, contrib)
                d = solve(A, bv, damp)
                if d is None:
                    ok = False
                else:
                    R, t = R.copy(), t.copy()
                    for f in range(1, tl):
                        R[f], t[f] = exp_update(d[6 * (f - 1):6 * f], R[f], t[f])
                    out['steps'][b] += 1
        ps = np.zeros((tl, tl, 4))
        ps[np.eye(tl, dtype=bool)] = [0, 0, 0, 1]
        tn = tw = tc = 0.0
        for (i, j) in trk.pairs:                                  # ascending (i, j)
            nc, sw, sc = sums[(i, j)][29], sums[(i, j)][27], sums[(i, j)][28]
            c = (i, j) in contrib
            ps[i, j] = [nc, sw / nc if nc > 0 else 0.0, np.sqrt(sc / sw) if (nc > 0 and sw > 0) else 0.0, 1.0 if c else 0.0]
            if c:
                tn, tw, tc = tn + nc, tw + sw, tc + sc
        out['state_R'][b], out['state_t'][b] = R, t
        out['R'][b], out['t'][b], out['pair_stats'][b] = R, t, ps
        out['track_stats'][b] = [len(contrib), tn, np.sqrt(tc / tw) if tw > 0 else 0.0, 1.0 if ok else 0.0]
    return out
