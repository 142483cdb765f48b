"""Numpy restatement of dis_tsdf_raycast (include/dis_hip.h, section "volumetric fusion") - and nothing else: the plain march, every
sample of every ray, no skipping.  Parameterised by dtype like tests/tsdf_ref.py: the same code runs in float64 (the oracle) and in
float32 (the kernel's arithmetic); the distance between the two gives the tests their tolerance (tsdf_ref.tolerance) and `exempt` the
pixels whose decisions may fall either way.  Every expression is written in the operand order csrc/raycast.hip follows."""
import numpy as np

from tests import tsdf_ref

MAX_N = 2 ** 24 - 1


def view_range(origin, voxel, grid, R, t, step):
    """the sample indices between the nearest and the farthest corner of the lattice box in the view R, t (float64), one more on
    either side: a sample outside the box is invalid, so a wider range changes nothing.  -> (n0, n1), empty when n1 < n0"""
    nx, ny, nz = grid
    o = np.asarray(origin, dtype=np.float64)
    ext = np.array([nx - 1, ny - 1, nz - 1], dtype=np.float64) * float(voxel)
    X = np.array([o + ext * np.array([i, j, k]) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    z = X @ np.asarray(R, dtype=np.float64)[2] + float(t[2])
    n0 = max(1, int(np.floor(z.min() / float(step))) - 1)
    n1 = min(MAX_N, int(np.ceil(z.max() / float(step))) + 1)
    return n0, n1


def _lerp(a, b, f):
    return a + f * (b - a)


def cast(tsdf, weight, vvalue, origin, voxel, R, t, K, baseline, size, step=None, min_weight=1, dtype=np.float64):
    """tsdf, weight, vvalue (nz, ny, nx), origin (3), R (nv, 3, 3), t (nv, 3), K (3, 3), size (h, w) -> dict
        disp (nv, h, w), normal (nv, 3, h, w), value (nv, h, w), hit (nv, h, w) bool, nstar (nv, h, w) int (0: none)
        views: per view a dict n0, and per sample of the walked range, shape (N, h w): cell (the linear cell index, -1 outside the
        lattice), valid, s (0 where not valid), edge (the sample lies within the rounding band of a cell boundary whose two cells
        differ in validity: see `exempt`)"""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    nz, ny, nx = tsdf.shape
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    F = tsdf.astype(dt)
    V = np.asarray(vvalue, dtype=np.float32).astype(dt)
    okw = np.asarray(weight, dtype=np.uint8) >= int(min_weight)
    Rv = np.asarray(R, dtype=np.float32).astype(dt)
    tv = np.asarray(t, dtype=np.float32).astype(dt)
    fx, fy, cx, cy = f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2])
    fb = dt(np.float32(K[0][0]) * np.float32(baseline))            # formed in fp32 on the host
    vx = f32(voxel)
    st = vx if step is None else f32(step)
    org = [f32(origin[k]) for k in range(3)]
    h, w = int(size[0]), int(size[1])
    nv, P = len(Rv), h * w
    vv, uu = np.indices((h, w))
    dc0, dc1 = (uu.reshape(-1).astype(dt) - cx) / fx, (vv.reshape(-1).astype(dt) - cy) / fy
    lim = (nx - 1, ny - 1, nz - 1)
    # the validity of every cell, with a layer of invalid cells around the lattice
    cv = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        cv &= okw[(c >> 2):(c >> 2) + nz - 1, ((c >> 1) & 1):((c >> 1) & 1) + ny - 1, (c & 1):(c & 1) + nx - 1]
    cvp = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    cvp[1:-1, 1:-1, 1:-1] = cv
    out = {'disp': np.zeros((nv, P), dt), 'normal': np.zeros((nv, 3, P), dt), 'value': np.zeros((nv, P), dt), 'hit': np.zeros((nv, P), bool),
           'nstar': np.zeros((nv, P), np.int64), 'views': []}
    cols = np.arange(P)
    with np.errstate(all='ignore'):
        for f in range(nv):
            Rf, tf = Rv[f], tv[f]
            o = [-((Rf[0, k] * tf[0] + Rf[1, k] * tf[1]) + Rf[2, k] * tf[2]) for k in range(3)]
            d = [(Rf[0, k] * dc0 + Rf[1, k] * dc1) + Rf[2, k] for k in range(3)]
            n0, n1 = view_range([np.float32(v) for v in origin], np.float32(voxel), (nx, ny, nz), np.asarray(R, dtype=np.float32)[f],
                                np.asarray(t, dtype=np.float32)[f], np.float32(voxel if step is None else step))
            ns = np.arange(n0, max(n1, n0 - 1) + 1)
            z = ns.astype(dt)[:, None] * st                              # float(n) step, every sample on its own
            g = [((o[k] + z * d[k][None, :]) - org[k]) / vx for k in range(3)]
            inside = np.ones(g[0].shape, bool)
            for k in range(3):
                inside &= (g[k] >= 0) & (g[k] < dt(lim[k]))
            i = [np.where(inside, np.floor(g[k]), 0).astype(np.int64) for k in range(3)]
            fr = [g[k] - i[k].astype(dt) for k in range(3)]
            corner = lambda A, c: A[i[2] + (c >> 2), i[1] + ((c >> 1) & 1), i[0] + (c & 1)]
            valid = inside & cv[i[2], i[1], i[0]]

            def trilinear(A, ii, ff):
                C = [A[ii[2] + (c >> 2), ii[1] + ((c >> 1) & 1), ii[0] + (c & 1)] for c in range(8)]
                c00, c10, c01, c11 = (_lerp(C[0], C[1], ff[0]), _lerp(C[2], C[3], ff[0]), _lerp(C[4], C[5], ff[0]), _lerp(C[6], C[7], ff[0]))
                return _lerp(_lerp(c00, c10, ff[1]), _lerp(c01, c11, ff[1]), ff[2]), C

            s = np.where(valid, trilinear(F, i, fr)[0], dt(0))
            neg = valid & (s < 0)
            has = neg.any(axis=0) if len(ns) else np.zeros(P, bool)
            idx = neg.argmax(axis=0) if len(ns) else np.zeros(P, np.int64)
            nstar = np.where(has, n0 + idx, 0)
            before = np.maximum(idx - 1, 0)
            hit = has & (idx >= 1) & (nstar >= 2)                        # (the sample before the walked range lies outside the box)
            if len(ns):
                s0, s1 = s[before, cols], s[idx, cols]
                hit &= valid[before, cols] & (s0 >= 0)
                zs = (nstar - 1).astype(dt) * st + st * (s0 / np.where(hit, s0 - s1, dt(1)))
                out['disp'][f] = np.where(hit, fb / np.where(hit, zs, dt(1)), dt(0))
                # normal and value at sample n*, in its cell
                ii = [a[idx, cols] for a in i]
                ff = [a[idx, cols] for a in fr]
                _, C = trilinear(F, ii, ff)
                dx00, dx10, dx01, dx11 = C[1] - C[0], C[3] - C[2], C[5] - C[4], C[7] - C[6]
                c00, c10, c01, c11 = C[0] + ff[0] * dx00, C[2] + ff[0] * dx10, C[4] + ff[0] * dx01, C[6] + ff[0] * dx11
                gx0, gx1 = dx00 + ff[1] * (dx10 - dx00), dx01 + ff[1] * (dx11 - dx01)
                dy0, dy1 = c10 - c00, c11 - c01
                c0, c1 = c00 + ff[1] * dy0, c01 + ff[1] * dy1
                gr = [gx0 + ff[2] * (gx1 - gx0), dy0 + ff[2] * (dy1 - dy0), c1 - c0]
                ln = np.sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2])
                okn = hit & (ln > 0) & np.isfinite(ln)
                for k in range(3):
                    out['normal'][f, k] = np.where(okn, gr[k] / np.where(okn, ln, dt(1)), dt(0))
                out['value'][f] = np.where(hit, trilinear(V, ii, ff)[0], dt(0))
            out['hit'][f], out['nstar'][f] = hit, nstar
            # the rounding band of a lattice coordinate: it is formed by at most 17 roundings (2 in dc, 5 in d, 5 in o, z, z d, the sum,
            # the difference, the quotient), each at most 2^-24 of M_a = sum |R[j][a] t_j| + z sum |R[j][a] dc_j| + |origin_a|, taken
            # in lattice units: below 16 2^-23 M_a / voxel.  Within that band of an integer the cell may be either neighbour.
            edge = np.zeros(g[0].shape, bool)
            nearn = np.zeros(g[0].shape, np.int64)
            base = [np.clip(np.floor(g[k]), -1, lim[k]).astype(np.int64) + 1 for k in range(3)]
            for a in range(3):
                M = ((abs(Rf[0, a] * tf[0]) + abs(Rf[1, a] * tf[1]) + abs(Rf[2, a] * tf[2]))
                     + z * (np.abs(Rf[0, a] * dc0) + np.abs(Rf[1, a] * dc1) + abs(Rf[2, a]))[None, :] + abs(org[a]))
                r = np.rint(g[a])
                near = np.abs(g[a] - r) <= 16.0 * 2.0 ** -23 * (M / vx)
                lo = [b for b in base]
                hi = [b for b in base]
                lo[a] = np.clip(r - 1, -1, lim[a]).astype(np.int64) + 1
                hi[a] = np.clip(r, -1, lim[a]).astype(np.int64) + 1
                edge |= near & (cvp[lo[2], lo[1], lo[0]] != cvp[hi[2], hi[1], hi[0]])
                nearn += near
            edge |= nearn >= 2                                           # near an edge or a corner of the lattice: any of four or eight cells
            cell = np.where(inside, (i[2] * (ny - 1) + i[1]) * (nx - 1) + i[0], -1).astype(np.int32)
            out['views'].append({'n0': n0, 'cell': cell, 'valid': valid, 's': s, 'edge': edge})
    for k in ('disp', 'value', 'hit', 'nstar'):
        out[k] = out[k].reshape(nv, h, w)
    out['normal'] = out['normal'].reshape(nv, 3, h, w)
    return out


def exempt(r32, r64):
    """-> (nv, h, w) bool: the pixels where float32 may legitimately decide differently from float64.  A pixel is exempt when
      - the two dtypes disagree about the hit or about n*;
      - or, among its samples up to n* of float64 (all of them where there is none),
          - one lies in another cell, or is inside or valid in one dtype only;
          - a valid one has |s64| within tsdf_ref.tolerance(s32, s64) - over those of these samples that are valid in the same cell in
            both dtypes; what lies behind n* takes part in no decision - of 0: the sign hangs on roundoff;
          - one lies within the rounding band of a cell boundary (see `cast`) whose two cells differ in validity."""
    nv, h, w = r64['hit'].shape
    ex = ((r32['hit'] != r64['hit']) | (r32['nstar'] != r64['nstar'])).reshape(nv, -1)
    nst = r64['nstar'].reshape(nv, -1)
    upto, a32, a64 = [], [], []
    for f, (v32, v64) in enumerate(zip(r32['views'], r64['views'])):
        ns = v64['n0'] + np.arange(v64['cell'].shape[0])
        upto.append((ns[:, None] <= nst[f][None, :]) | (nst[f] == 0)[None, :])
        both = v32['valid'] & v64['valid'] & (v32['cell'] == v64['cell']) & upto[f]
        a32.append(v32['s'][both])
        a64.append(v64['s'][both])
    band = tsdf_ref.tolerance(np.concatenate(a32), np.concatenate(a64)) if a32 else 0.0
    for f, (v32, v64) in enumerate(zip(r32['views'], r64['views'])):
        if not v64['cell'].shape[0]:
            continue
        differ = (v32['cell'] != v64['cell']) | (v32['valid'] != v64['valid'])
        close = v64['valid'] & (np.abs(v64['s']) <= band)
        ex[f] |= ((differ | close | v64['edge']) & upto[f]).any(axis=0)
    return ex.reshape(nv, h, w)
