"""Numpy restatement of the volumetric fusion (include/dis_hip.h, section "volumetric fusion") - and nothing else.  Parameterised by
dtype: the same code runs in float64 (the oracle) and in float32 (what the kernels' arithmetic is; the distance between the two gives
the tests their tolerance and the band inside which a decision may fall either way).  Every sum is written in an explicit operand
order, which csrc/tsdf.hip follows."""
import numpy as np


def _valid(d):
    return np.isfinite(d) & (d > 0)


def integrate(disp, R, t, K, baseline, value, origin, voxel, trunc, grid, dtype=np.float64):
    """disp (tl, H, W) float32, R (tl, 3, 3), t (tl, 3), K (3, 3), value (tl, H, W) or None, origin (3), grid (nx, ny, nz) -> dict
        tsdf (nz, ny, nx), weight (nz, ny, nx) uint8, vvalue (nz, ny, nx)
        per (frame, lattice point), shape (tl, nz, ny, nx): front (z > 0), su, sv (u + 0.5, v + 0.5; 0 where not front), pu, pv (their
        floors), inimg (front and the pixel inside the image), ok (inimg and a valid disparity), sdf (0 where not ok), use (the frame
        adds to tsdf and weight), vuse (it adds to vvalue)"""
    disp = np.asarray(disp, dtype=np.float32)
    tl, H, W = disp.shape
    nx, ny, nz = (int(g) for g in grid)
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    R = np.asarray(R, dtype=np.float32).astype(dt)
    t = np.asarray(t, dtype=np.float32).astype(dt)
    fx, fy, cx, cy = f32(K[0][0]), f32(K[1][1]), f32(K[0][2]), f32(K[1][2])
    fb = dt(np.float32(K[0][0]) * np.float32(baseline))            # formed in fp32 on the host
    vx, tr = f32(voxel), f32(trunc)
    val = np.zeros((tl, H, W), dt) if value is None else np.asarray(value, dtype=np.float32).reshape(tl, H, W).astype(dt)
    X = [(f32(origin[0]) + np.arange(nx, dtype=dt) * vx)[None, None, :], (f32(origin[1]) + np.arange(ny, dtype=dt) * vx)[None, :, None],
         (f32(origin[2]) + np.arange(nz, dtype=dt) * vx)[:, None, None]]
    shape = (nz, ny, nx)
    acc, vsum = np.zeros(shape, dt), np.zeros(shape, dt)
    weight, vcnt = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    out = {k: np.zeros((tl,) + shape, bool) for k in ('front', 'inimg', 'ok', 'use', 'vuse')}
    out.update({k: np.zeros((tl,) + shape, dt) for k in ('su', 'sv', 'pu', 'pv', 'sdf')})
    with np.errstate(all='ignore'):
        for f in range(tl):
            Xc = [((R[f, r, 0] * X[0] + R[f, r, 1] * X[1]) + R[f, r, 2] * X[2]) + t[f, r] for r in range(3)]
            z = Xc[2]
            front = z > 0
            zs = np.where(front, z, dt(1))
            su = np.where(front, (fx * (Xc[0] / zs) + cx) + dt(0.5), dt(0))
            sv = np.where(front, (fy * (Xc[1] / zs) + cy) + dt(0.5), dt(0))
            pu, pv = np.floor(su), np.floor(sv)
            inimg = front & (pu >= 0) & (pu <= dt(W - 1)) & (pv >= 0) & (pv <= dt(H - 1))
            iu, iv = np.where(inimg, pu, 0).astype(np.int64), np.where(inimg, pv, 0).astype(np.int64)
            d = disp[f][iv, iu]
            ok = inimg & _valid(d)
            depth = fb / np.where(ok, d, np.float32(1)).astype(dt)
            sdf = np.where(ok, depth - z, dt(0))
            use = ok & ~(sdf < -tr)
            acc = np.where(use, acc + np.minimum(sdf / tr, dt(1)), acc)
            weight += use
            vuse = use & (sdf <= tr)
            vsum = np.where(vuse, vsum + val[f][iv, iu], vsum)
            vcnt += vuse
            for k, a in (('front', front), ('inimg', inimg), ('ok', ok), ('use', use), ('vuse', vuse), ('su', su), ('sv', sv), ('pu', pu),
                         ('pv', pv), ('sdf', sdf)):
                out[k][f] = a
        out['tsdf'] = np.where(weight > 0, acc / np.maximum(weight, 1).astype(dt), dt(1))
        out['vvalue'] = np.where(vcnt > 0, vsum / np.maximum(vcnt, 1).astype(dt), dt(0))
    out['weight'] = weight.astype(np.uint8)
    out['image'], out['trunc'] = (H, W), float(np.float32(trunc))
    return out


def tolerance(r32, r64):
    """what the device may deviate from r64 in a float output: 16 max|r32 - r64| + 16 2^-23 max(1, max|r64|)  (the rule of fuse_ref)"""
    r64 = np.asarray(r64, dtype=np.float64)
    d = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max()) if r64.size else 0.0
    return 16.0 * d + 16.0 * 2.0 ** -23 * max(1.0, float(np.abs(r64).max()) if r64.size else 0.0)


def exempt(r32, r64):
    """-> (points (nz, ny, nx) bool, pairs (tl, nz, ny, nx) bool): where float32 may legitimately decide differently from float64.
    A (frame, lattice point) pair is exempt when
      - the two dtypes choose another pixel for it, or take its skip / use decision (for tsdf and weight, or for vvalue) differently;
      - or, lying in front of the camera and within a pixel of the image, s = u + 0.5 (or v + 0.5) lies within the band
        16 max|s32 - s64| + 16 2^-23 (the maximum over such pairs, for each axis on its own) of an integer: the rounding boundaries
        between pixels and at the image edges;
      - or its sdf, where float64 reaches one, lies within the band tolerance(sdf32, sdf64) (over the pairs that reach one at the same
        pixel in both) of -trunc or of +trunc.
    A lattice point is exempt when one of its pairs is, or when |tsdf64| lies within tolerance(tsdf32, tsdf64) (over the other points)
    of 0: its sign hangs on roundoff."""
    H, W = r64['image']
    tr = np.float64(r64['trunc'])
    pairs = (r32['use'] != r64['use']) | (r32['vuse'] != r64['vuse']) | (r32['inimg'] != r64['inimg'])
    same_px = (r32['pu'].astype(np.float64) == r64['pu']) & (r32['pv'].astype(np.float64) == r64['pv'])
    pairs |= r32['inimg'] & r64['inimg'] & ~same_px
    near = r64['front'] & r32['front'] & (r64['su'] >= -1.0) & (r64['su'] <= W + 1.0) & (r64['sv'] >= -1.0) & (r64['sv'] <= H + 1.0)
    for key in ('su', 'sv'):
        if near.any():
            # the rule of `tolerance` applied to the quantity the choice hangs on, the signed distance from the nearest boundary
            # (at most 1 / 2 in size, and off by s32 - s64 between the dtypes)
            band_p = 16.0 * float(np.abs(r32[key].astype(np.float64) - r64[key])[near].max()) + 16.0 * 2.0 ** -23
            pairs |= near & (np.abs(r64[key] - np.rint(r64[key])) <= band_p)
    both = r32['ok'] & r64['ok'] & same_px
    band_s = tolerance(r32['sdf'][both], r64['sdf'][both])
    pairs |= r64['ok'] & ((np.abs(r64['sdf'] + tr) <= band_s) | (np.abs(r64['sdf'] - tr) <= band_s))
    points = pairs.any(axis=0)
    m = ~points
    band_t = tolerance(r32['tsdf'][m], r64['tsdf'][m])
    points = points | ((r64['weight'] > 0) & (np.abs(r64['tsdf']) <= band_t))
    return points, pairs


_PQ = ((0, 0), (0, 1), (1, 0), (1, 1))
_QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))


def extract(tsdf, weight, vvalue, origin, voxel, min_weight=1, dtype=np.float64):
    """naive surface nets of the volume tsdf, weight, vvalue (nz, ny, nx) -> dict: xyz, normal (V, 3), value (V), views (V) uint8,
    cell (V) int32 (ascending linear cell indices), faces (M, 3) int32, vid (nz - 1, ny - 1, nx - 1) int32 (-1: inactive),
    count = [V, M]"""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    weight = np.asarray(weight, dtype=np.uint8)
    nz, ny, nx = tsdf.shape
    dt = np.dtype(dtype).type
    f32 = lambda x: dt(np.float32(x))
    F = tsdf.astype(dt)
    V = np.asarray(vvalue, dtype=np.float32).astype(dt)
    neg = tsdf < 0
    okw = weight >= int(min_weight)
    cz, cy, cx = nz - 1, ny - 1, nx - 1

    def corner(A, c):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        return A[dz:dz + cz, dy:dy + cy, dx:dx + cx]

    allok = np.ones((cz, cy, cx), bool)
    nneg = np.zeros((cz, cy, cx), np.int64)
    for c in range(8):
        allok &= corner(okw, c)
        nneg += corner(neg, c)
    active = allok & (nneg > 0) & (nneg < 8)
    sums = [np.zeros((cz, cy, cx), dt) for _ in range(3)]
    cnt = np.zeros((cz, cy, cx), np.int64)
    g = [None] * 3
    with np.errstate(all='ignore'):
        for a in range(3):
            b, c_ = (a + 1) % 3, (a + 2) % 3
            for p, q in _PQ:
                off = [0, 0, 0]
                off[b], off[c_] = p, q
                lo = off[0] | (off[1] << 1) | (off[2] << 2)
                hi = lo | (1 << a)
                fa, fb = corner(F, lo), corner(F, hi)
                cross = corner(neg, lo) != corner(neg, hi)
                pt = [None] * 3
                pt[a], pt[b], pt[c_] = fa / np.where(cross, fa - fb, dt(1)), dt(p), dt(q)
                for k in range(3):
                    sums[k] = np.where(cross, sums[k] + pt[k], sums[k])
                cnt += cross
                g[a] = (fb - fa) if g[a] is None else g[a] + (fb - fa)
        nc = np.maximum(cnt, 1).astype(dt)
        kk, jj, ii = np.indices((cz, cy, cx))
        xyz = [f32(origin[k]) + (idx.astype(dt) + sums[k] / nc) * f32(voxel) for k, idx in enumerate((ii, jj, kk))]
        ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        okn = (ln > 0) & np.isfinite(ln)
        nrm = [np.where(okn, gc / np.where(okn, ln, dt(1)), dt(0)) for gc in g]
        vs = corner(V, 0)
        views = corner(weight, 0)
        for c in range(1, 8):
            vs = vs + corner(V, c)
            views = np.minimum(views, corner(weight, c))
        vs = vs / dt(8)
    sel = np.flatnonzero(active.reshape(-1))
    vid = np.full(cz * cy * cx, -1, np.int32)
    vid[sel] = np.arange(len(sel), dtype=np.int32)
    vid = vid.reshape(cz, cy, cx)
    out = {'xyz': np.stack([x.reshape(-1)[sel] for x in xyz], 1), 'normal': np.stack([x.reshape(-1)[sel] for x in nrm], 1),
           'value': vs.reshape(-1)[sel], 'views': views.reshape(-1)[sel].astype(np.uint8), 'cell': sel.astype(np.int32), 'vid': vid}
    # faces: one quad per lattice edge whose ends differ in sign and whose four cells are active
    n = (nx, ny, nz)
    K_, J_, I_ = np.indices((nz, ny, nx))
    coords = (I_.reshape(-1), J_.reshape(-1), K_.reshape(-1))
    negf, posf = neg.reshape(-1), ~neg.reshape(-1)
    stride = (1, nx, nx * ny)
    keys, quads = [], []
    for a in range(3):
        b, c_ = (a + 1) % 3, (a + 2) % 3
        if n[b] < 3 or n[c_] < 3:
            continue
        cond = ((coords[a] <= n[a] - 2) & (coords[b] >= 1) & (coords[b] <= n[b] - 2) & (coords[c_] >= 1) & (coords[c_] <= n[c_] - 2))
        lin = np.flatnonzero(cond)
        lin = lin[negf[lin] != negf[lin + stride[a]]]
        q = []
        for ob, oc in _QUAD:
            cc = [coords[0][lin], coords[1][lin], coords[2][lin]]
            cc[b] = cc[b] + ob
            cc[c_] = cc[c_] + oc
            q.append(vid[cc[2], cc[1], cc[0]])
        q = np.stack(q, 1) if len(lin) else np.zeros((0, 4), np.int32)
        good = (q >= 0).all(1)
        lin, q = lin[good], q[good]
        rev = posf[lin]
        q[rev] = q[rev][:, ::-1]
        keys.append(lin * 3 + a)
        quads.append(q)
    if keys:
        keys, quads = np.concatenate(keys), np.concatenate(quads)
        quads = quads[np.argsort(keys, kind='stable')]
    else:
        quads = np.zeros((0, 4), np.int32)
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    out['faces'] = faces
    out['count'] = np.array([len(sel), len(faces)], np.int32)
    return out
