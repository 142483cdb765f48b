"""Numpy restatement of dis_tsdf_align_poses (include/dis_hip.h, section "volumetric fusion") - and nothing else.  Parameterised by
dtype like tests/pose_ref.py: float64 is the oracle; float32 forms every per-pixel term in float32 and adds the terms in float64, which
is what csrc/tsdf_align.hip does (the state and the solve are float64 in both: pose_ref.solve_step).  Every per-pixel expression is
written in the operand order of the kernel: the sampler is the one of tests/raycast_ref.py."""
import numpy as np

from tests import pose_ref

NSUMS = pose_ref.NSUMS
hidx = pose_ref.hidx


def _lerp(a, b, f):
    return a + f * (b - a)


def _stats3(S):
    nc, sw, sc = S[29], S[27], S[28]
    return [nc, sw / nc if nc > 0 else 0.0, np.sqrt(sc / sw) if (nc > 0 and sw > 0) else 0.0]


def view_sums(F, cv, org, vx, tr, tv, s2, R, t, P, dt):
    """the 30 sums of one pass of one view at the state (R, t) (float64; its rounding to dt is used).  F (nz, ny, nx) in dt, cv the
    validity of the cells, P the view's back-projected valid pixels (3 arrays in dt) -> float64 (30,)"""
    nz, ny, nx = F.shape
    Rs, ts = R.astype(dt), t.astype(dt)
    q = [P[k] - ts[k] for k in range(3)]
    X = [(Rs[0, k] * q[0] + Rs[1, k] * q[1]) + Rs[2, k] * q[2] for k in range(3)]
    g = [(X[k] - org[k]) / vx for k in range(3)]
    lim = (nx - 1, ny - 1, nz - 1)
    inside = np.ones(g[0].shape, bool)
    for k in range(3):
        inside &= (g[k] >= 0) & (g[k] < dt(lim[k]))
    i = [np.where(inside, np.floor(g[k]), 0).astype(np.int64) for k in range(3)]
    use = inside & cv[i[2], i[1], i[0]]
    i = [a[use] for a in i]
    f = [g[k][use] - i[k].astype(dt) for k in range(3)]
    C = [F[i[2] + (c >> 2), i[1] + ((c >> 1) & 1), i[0] + (c & 1)] for c in range(8)]
    c00, c10, c01, c11 = _lerp(C[0], C[1], f[0]), _lerp(C[2], C[3], f[0]), _lerp(C[4], C[5], f[0]), _lerp(C[6], C[7], f[0])
    s = _lerp(_lerp(c00, c10, f[1]), _lerp(c01, c11, f[1]), f[2])
    # the gradient of the interpolant, in the operand order of raycast_ref.cast
    dx00, dx10, dx01, dx11 = C[1] - C[0], C[3] - C[2], C[5] - C[4], C[7] - C[6]
    c00, c10, c01, c11 = C[0] + f[0] * dx00, C[2] + f[0] * dx10, C[4] + f[0] * dx01, C[6] + f[0] * dx11
    gx0, gx1 = dx00 + f[1] * (dx10 - dx00), dx01 + f[1] * (dx11 - dx01)
    dy0, dy1 = c10 - c00, c11 - c01
    c0, c1 = c00 + f[1] * dy0, c01 + f[1] * dy1
    gr = [gx0 + f[2] * (gx1 - gx0), dy0 + f[2] * (dy1 - dy0), c1 - c0]
    near = np.abs(s) < 1
    s = s[near]
    gr = [a[near] for a in gr]
    Pu = [P[k][use][near] for k in range(3)]
    e = tr * s
    m = [tv * a for a in gr]
    n = [(Rs[r, 0] * m[0] + Rs[r, 1] * m[1]) + Rs[r, 2] * m[2] for r in range(3)]
    J = [n[1] * Pu[2] - n[2] * Pu[1], n[2] * Pu[0] - n[0] * Pu[2], n[0] * Pu[1] - n[1] * Pu[0], -n[0], -n[1], -n[2]]
    e2 = e * e
    gw = dt(1) / (dt(1) + e2 / s2)
    w = gw * gw
    S = np.zeros(NSUMS, np.float64)
    f64sum = lambda x: float(np.sum(x.astype(np.float64)))
    for p in range(6):
        wJ = w * J[p]
        for q_ in range(p, 6):
            S[hidx(p, q_)] = f64sum(wJ * J[q_])
        S[21 + p] = f64sum(wJ * e)
    S[27] = f64sum(w)
    S[28] = f64sum(w * e2)
    S[29] = float(s.size)
    return S


def align(tsdf, weight, origin, voxel, trunc, disp, K, baseline, R_init, t_init, iters=6, scale=None, damping=0.0, min_corr=64, min_weight=1,
          dtype=np.float64):
    """tsdf, weight (nz, ny, nx), origin (3), disp (nv, H, W), K (3, 3), R_init (nv, 3, 3), t_init (nv, 3) -> dict
        R (nv, 3, 3), t (nv, 3), stats (nv, 8): the float64 state and statistics rounded to dtype
        state_R, state_t: the float64 state itself
        sums (nv, iters + 1, 30): the sums of every pass, the closing one included; steps (nv): how many steps were taken"""
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    F = np.asarray(tsdf, dtype=np.float32).astype(dt)
    nz, ny, nx = F.shape
    okw = np.asarray(weight, dtype=np.uint8) >= int(min_weight)
    cv = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        cv &= okw[(c >> 2):(c >> 2) + nz - 1, ((c >> 1) & 1):((c >> 1) & 1) + ny - 1, (c & 1):(c & 1) + nx - 1]
    disp = np.asarray(disp, dtype=np.float32)
    disp = disp.reshape(disp.shape[0], disp.shape[-2], disp.shape[-1])
    nv, H, W = disp.shape
    fx, fy, cx, cy = f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2])
    fb = dt(np.float32(np.float32(K[0][0]) * np.float32(baseline)))     # the device forms these three in float32 on the host
    sc = np.float32(trunc / 2 if scale is None else scale)
    s2 = dt(np.float32(sc * sc))
    tv = dt(np.float32(np.float32(trunc) / np.float32(voxel)))
    vx, tr = f32(voxel), f32(trunc)
    org = [f32(origin[k]) for k in range(3)]
    damp = float(np.float32(damping))
    R_init, t_init = np.asarray(R_init, dtype=np.float32), np.asarray(t_init, dtype=np.float32)
    out = {'R': np.zeros((nv, 3, 3), dt), 't': np.zeros((nv, 3), dt), 'stats': np.zeros((nv, 8), dt), 'state_R': np.zeros((nv, 3, 3)),
           'state_t': np.zeros((nv, 3)), 'sums': np.zeros((nv, iters + 1, NSUMS)), 'steps': np.zeros(nv, np.int64)}
    with np.errstate(all='ignore'):
        for f in range(nv):
            d = disp[f]
            ok = np.isfinite(d) & (d > 0)
            v, u = np.nonzero(ok)
            z = fb / d[ok].astype(dt)
            P = [z * ((u.astype(dt) - cx) / fx), z * ((v.astype(dt) - cy) / fy), z]
            R, t, good = R_init[f].astype(np.float64), t_init[f].astype(np.float64), True
            for k in range(iters + 1):
                S = view_sums(F, cv, org, vx, tr, tv, s2, R, t, P, dt)
                out['sums'][f, k] = S
                if k == 0:
                    opening = _stats3(S)
                if k < iters and good:
                    R, t, good = pose_ref.solve_step(S, R, t, damp, min_corr)
                    out['steps'][f] += good
            out['state_R'][f], out['state_t'][f] = R, t
            out['R'][f], out['t'][f] = R, t
            out['stats'][f] = _stats3(S) + [1.0 if good else 0.0] + opening + [float(ok.sum())]
    return out


def tolerance(r32, r64):
    return pose_ref.tolerance(r32, r64)


def pose_error(R, t, R_true, t_true):
    """the rotation angle of R R_true^T in radians and |t - R R_true^T t_true|: how far the camera frame of (R, t) is from the true one"""
    R, t, Rt, tt = (np.asarray(a, dtype=np.float64) for a in (R, t, R_true, t_true))
    dR = R @ Rt.T
    s = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(dR) - 1.0))), float(np.linalg.norm(t - dR @ tt))
