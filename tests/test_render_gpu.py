"""GPU: dis_render_track (csrc/render.hip) against the fp64 oracle of tests/render_ref.py.

Tolerances.  The oracle's own arithmetic was run in float32 numpy on the three scenes of test 1 and compared with float64 on the
non-ambiguous pixels; the constants below are 4x the largest deviation seen (the margin is for operation order and fused rounding):
    disp     1.56e-05 (seeds 1, 2, 3: 7.28e-06, 2.96e-06, 1.56e-05)   ambient  2.23e-07 (1.90e-07, 2.23e-07, 1.62e-07)
    im       1.62e-06 (1.62e-06, 8.95e-07, 8.26e-07)                  flow     1.29e-05 (1.29e-05, 1.06e-05, 9.19e-06)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import render_ref, render_scenes

pytestmark = pytest.mark.gpu

TOL = {'disp': 4 * 1.56e-05, 'ambient': 4 * 2.23e-07, 'im': 4 * 1.62e-06, 'flow': 4 * 1.29e-05}
_REF = {}


def _render(scene, settings, want_ids=True):
    from depthinspace_amd import ops
    verts, faces, albedo, R, t, blend = scene
    dev = torch.device('cuda')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pattern = up(np.ascontiguousarray(settings.pattern[..., 0], dtype=np.float32))
    res = ops.render_track(up(verts), up(faces), up(albedo), up(R), up(t), settings.K, settings.baseline, blend, pattern,
                           want_ids=want_ids)
    torch.cuda.synchronize()
    return res


def _small_ref(seed):
    """the fp64 oracle of small_scene(seed): computed once, shared, never modified"""
    if seed not in _REF:
        st = render_scenes.small_settings()
        sc = render_scenes.small_scene(seed)
        _REF[seed] = (st, sc, render_ref.render_ref(*sc[:5], st.K, st.baseline, sc[5], st.pattern[..., 0]))
    return _REF[seed]


def _flat(x, tl):
    return x.detach().cpu().numpy().reshape(tl, -1)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_against_fp64_oracle(seed):
    st, sc, ref = _small_ref(seed)
    tl = 3
    res = _render(sc, st)
    ok = ~ref['ambiguous']
    shadow = (ref['tri_id'] >= 0) & (ref['lit'] == 0)
    print(f'seed {seed}: ambiguous {ref["ambiguous"].mean():.4f} shadowed {shadow.mean():.4f} object {(ref["tri_id"] >= 2).mean():.4f}')
    assert ref['ambiguous'].mean() <= 0.03 and shadow.mean() >= 0.01 and (ref['tri_id'] >= 2).mean() >= 0.10
    tid, lit = _flat(res['tri_id'], tl), _flat(res['lit'], tl)
    print('tri_id mismatches', int((tid != ref['tri_id'])[ok].sum()), 'lit mismatches', int((lit != ref['lit'])[ok].sum()))
    assert np.array_equal(tid[ok], ref['tri_id'][ok])
    assert np.array_equal(lit[ok], ref['lit'][ok])
    for k in ('disp', 'ambient', 'im'):
        err = np.abs(_flat(res[k], tl).astype(np.float64) - ref[k])[ok].max()
        print(k, 'max error', err, 'bound', TOL[k])
        assert err <= TOL[k], (k, err)
    flow = res['flow'].detach().cpu().numpy().reshape(tl, tl, 2, -1).astype(np.float64)
    err = np.abs(flow - ref['flow'])[np.broadcast_to(ok[:, None, None, :], flow.shape)].max()
    print('flow max error', err, 'bound', TOL['flow'])
    assert err <= TOL['flow'], err
    for i in range(tl):
        assert not flow[i, i].any()
    # a miss does not exist in these scenes (the board fills the view); the outputs are finite everywhere
    assert all(bool(torch.isfinite(res[k]).all()) for k in ('im', 'ambient', 'disp', 'flow'))


def test_watertight_icosphere():
    """Every pixel whose ray meets the sphere inscribed in a 320-face icosphere must see the mesh, not the board behind it: the region
    holds every interior edge and vertex of the visible side.  (The inscribed radius is taken 1e-6 short: the float32 vertices the
    renderer is given lie within 1.2e-7 of the float64 ones.)"""
    st = render_scenes.small_settings(96, 96)
    centre, board_z = np.array([0.05, -0.03, 1.8]), 3.5
    verts, faces, albedo, R, t, r_in = render_scenes.sphere_scene(2, 0.5, centre, board_z)
    assert len(faces) == 2 + 320
    res = _render((verts, faces, albedo, R, t, 0.6), st)
    K = st.K.astype(np.float64)
    v, u = np.meshgrid(np.arange(96.0), np.arange(96.0), indexing='ij')
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    # |c - (c . d) d| < r: the ray from the origin meets the sphere of radius r about c
    dist = np.linalg.norm(centre[None, None] - (d @ centre)[..., None] * d, axis=-1)
    inside = dist < r_in - 1e-6
    assert inside.sum() > 1500
    depth = st.baseline * float(st.K[0, 0]) / res['disp'][0, 0].cpu().numpy().astype(np.float64)
    tid = res['tri_id'][0].cpu().numpy()
    assert (tid[inside] >= 2).all(), f'{int((tid[inside] < 2).sum())} rays slipped through the mesh'
    assert (depth[inside] < centre[2]).all() and (depth[inside] < board_z - 1).all()
    assert (tid[dist > 0.5 + 1e-6] < 2).all()      # and nothing outside the circumscribed sphere


@pytest.mark.parametrize('h,w,tl', [(64, 48, 3), (128, 96, 4)])
def test_plane_equals_synth(h, w, tl):
    """the CPU oracle test's comparison on the device; its tolerances (float32 poses against synth's fp64 ones, scaled by the focal
    length: 435 there) plus the float32 bounds of test 1"""
    from depthinspace_amd import synth
    st = render_scenes.small_settings(h, w, baseline=0.05)
    verts, faces, albedo, R, t, batch = render_scenes.plane_scene(st, tl, seed=7)
    res = _render((verts.astype(np.float32), faces, albedo, R, t, synth._BLEND), st)
    assert bool((res['tri_id'] >= 0).all()) and bool((res['lit'] == 1).all())
    assert np.abs(res['disp'].cpu().numpy()[:, 0] - batch['disp0'][0, :, 0]).max() < 1e-5 + TOL['disp']
    flow = res['flow'].cpu().numpy()
    for i in range(tl):
        for j in range(tl):
            if i != j:
                assert np.abs(flow[i * tl + j] - batch[f'flow_{i}{j}'][0, 0]).max() < 2e-4 + TOL['flow'], (i, j)


def test_culling_is_invisible():
    """~5 000 triangles at 96 x 80: sub-pixel triangles, a triangle nearer than the near distance, objects partly outside the frame.
    tri_id, lit and disp against the oracle on 2 000 random pixels; two renders are bit-identical."""
    st = render_scenes.small_settings(96, 80, baseline=0.2)
    sc = render_scenes.dense_scene()
    verts, faces = sc[0], sc[1]
    assert 4500 <= len(faces) <= 5500
    rng = np.random.RandomState(0)
    pix = rng.choice(96 * 80, 2000, replace=False)
    u, v = pix % 80, pix // 80
    ref = render_ref.render_ref(*sc[:5], st.K, st.baseline, sc[5], st.pattern[..., 0], pixels=(u, v), visibility=False)
    # the construction holds what the test is about
    K = st.K.astype(np.float64)
    tl = len(sc[3])
    Vc = verts.astype(np.float64) @ sc[3][0].astype(np.float64).T + sc[4][0].astype(np.float64)
    assert (Vc[faces[-1]][:, 2] < 0.05).all() and (Vc[faces[-1]][:, 2] > 0).all()                      # the near triangle
    uv = Vc[:, :2] / Vc[:, 2:3] * K[0, 0] + K[:2, 2]
    ext = np.ptp(uv[faces[2:-1]], axis=1).max(1)
    assert (ext < 1.0).sum() > 500                                                                        # sub-pixel triangles
    assert (uv[4:-3, 0] > 80).any() and (uv[4:-3, 0] < 0).any()                                           # partly outside
    a = _render(sc, st)
    b = _render(sc, st)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ok = ~ref['ambiguous']
    print('ambiguous', ref['ambiguous'].mean(), 'triangles seen', len(np.unique(ref['tri_id'])), 'shadowed', ((ref['lit'] == 0) & (ref['tri_id'] >= 0)).mean())
    assert ok.mean() > 0.8 and len(np.unique(ref['tri_id'])) > 300 and ((ref['lit'] == 0) & (ref['tri_id'] >= 0)).mean() > 0.01
    tid = a['tri_id'].cpu().numpy().reshape(tl, -1)[:, pix]
    lit = a['lit'].cpu().numpy().reshape(tl, -1)[:, pix]
    disp = a['disp'].cpu().numpy().reshape(tl, -1)[:, pix].astype(np.float64)
    print('tri_id mismatches', int((tid != ref['tri_id'])[ok].sum()), 'lit mismatches', int((lit != ref['lit'])[ok].sum()))
    assert np.array_equal(tid[ok], ref['tri_id'][ok])
    assert np.array_equal(lit[ok], ref['lit'][ok])
    err = np.abs(disp - ref['disp'])[ok].max()
    print('disp max error', err)
    assert err <= TOL['disp'], err


def test_geometry_closes_and_occlusion_exists():
    """Frame i's depth and flow i -> j, unprojected through R, t, land on frame j's surface where frame j sees the same point.
    Bound, per pixel: (1) both depths carry the disparity error of test 1: dz = z^2 / (b f) TOL['disp'] each, z the larger of the two.
    (2) Frame j's depth is sampled bilinearly; on one planar face 1 / z is affine in the pixel, so z_xx = 2 z_x^2 / z (and alike for
    yy, xy) and the bilinear error over a unit cell, (|z_xx| + |z_yy|) / 8 + |z_xy| / 4, is at most s^2 / z_min with s the spread of the
    four corner depths (s >= |z_x|, |z_y| across the cell).  (3) The sampling position is off by at most TOL['flow'] px in x and in
    y: 2 TOL['flow'] s.  So |z_reproj - z_sampled| <= 2 dz + s^2 / z_min + 2 TOL['flow'] s, checked where the oracle's visibility says
    frame j sees the point, all four corners show the triangle the oracle says the point is on, and nothing involved is ambiguous.
    Where the oracle says frame j does NOT see the point - silhouettes - the two depths must be far apart somewhere."""
    tl = 3
    st, sc, ref = _small_ref(1)
    res = _render(sc, st)
    H, W = st.imsize
    K = st.K.astype(np.float64)
    bf = st.baseline * K[0, 0]
    disp = res['disp'].cpu().numpy()[:, 0].astype(np.float64)
    tid = res['tri_id'].cpu().numpy()
    flow = res['flow'].cpu().numpy().astype(np.float64).reshape(tl, tl, 2, H, W)
    R, t = sc[3].astype(np.float64), sc[4].astype(np.float64)
    depth = bf / disp
    amb = ref['ambiguous'].reshape(tl, H, W)
    vis = ref['visible_in'].reshape(tl, tl, H, W)
    rid = ref['tri_id'].reshape(tl, H, W)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    n_closed = n_occluded = 0
    for i in range(tl):
        for j in range(tl):
            if i == j:
                continue
            Xc = np.stack([(u - K[0, 2]) / K[0, 0] * depth[i], (v - K[1, 2]) / K[1, 1] * depth[i], depth[i]], -1)
            Xj = ((Xc - t[i]) @ R[i]) @ R[j].T + t[j]
            uj, vj = u + flow[i, j, 0], v + flow[i, j, 1]
            inside = (uj >= 0) & (uj <= W - 1) & (vj >= 0) & (vj <= H - 1) & ~amb[i]
            x0, y0 = np.clip(np.floor(uj), 0, W - 2).astype(int), np.clip(np.floor(vj), 0, H - 2).astype(int)
            wx, wy = uj - x0, vj - y0
            c = [depth[j][y0, x0], depth[j][y0, x0 + 1], depth[j][y0 + 1, x0], depth[j][y0 + 1, x0 + 1]]
            zs = (c[0] * (1 - wx) + c[1] * wx) * (1 - wy) + (c[2] * (1 - wx) + c[3] * wx) * wy
            same = np.ones_like(inside)
            for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
                same &= (tid[j][yy, xx] == rid[i]) & ~amb[j][yy, xx]
            spread = np.max(c, 0) - np.min(c, 0)
            dz = np.maximum(Xj[..., 2], np.max(c, 0)) ** 2 / bf * TOL['disp']
            bound = 2 * dz + spread * spread / np.min(c, 0) + 2 * TOL['flow'] * spread
            sel = inside & vis[i, j] & same
            n_closed += int(sel.sum())
            bad = sel & (np.abs(Xj[..., 2] - zs) > bound)
            assert not bad.any(), (i, j, int(bad.sum()), float(np.abs(Xj[..., 2] - zs)[sel].max()))
            occ = inside & ~vis[i, j] & (np.abs(Xj[..., 2] - zs) > 0.05)
            n_occluded += int(occ.sum())
    print('pixels closing', n_closed, 'occluded', n_occluded)
    assert n_closed > 2000 and n_occluded > 20


def test_abi_behaviour():
    from depthinspace_amd import lib, ops
    st = render_scenes.small_settings()
    sc = render_scenes.small_scene(2)
    dev = torch.device('cuda')
    H, W = st.imsize
    tl, nv, nf = 3, len(sc[0]), len(sc[1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    verts, faces, albedo, R, t = (up(a) for a in sc[:5])
    pattern = up(np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32))
    K4 = lib.host_floats([st.K[0, 0], st.K[1, 1], st.K[0, 2], st.K[1, 2]])
    need = lib.fn('dis_render_workspace')(nv, nf, tl, H, W)
    assert need > 0 and lib.fn('dis_render_workspace')(nv, 0, tl, H, W) == -1 and lib.fn('dis_render_workspace')(nv, nf, 5, H, W) == -1
    assert lib.fn('dis_render_workspace')(nv, 65536, 4, 512, 432) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    POISON = float('nan')
    outs = {k: torch.full(s, POISON, device=dev) for k, s in (('im', (tl, 1, H, W)), ('ambient', (tl, 1, H, W)), ('disp', (tl, 1, H, W)),
                                                               ('flow', (tl * tl, 2, H, W)), ('lit', (tl, H, W)))}
    outs['tri_id'] = torch.full((tl, H, W), -12345, dtype=torch.int32, device=dev)
    O = lib.RenderOut()
    for k, _ in lib.RenderOut._fields_:
        setattr(O, k, outs[k].data_ptr())
    f = lib.fn('dis_render_track')
    s = torch.cuda.current_stream().cuda_stream
    p = lambda x: x.data_ptr()
    K4p, Op = ctypes.cast(K4, ctypes.c_void_p), ctypes.addressof(O)

    def call(verts_=p(verts), out_=Op, ws_=p(ws), nf_=nf, tl_=tl, h_=H):
        return f(verts_, p(faces), p(albedo), nv, nf_, p(R), p(t), K4p, st.baseline, sc[5], p(pattern), out_, tl_, h_, W, ws_, s)
    assert call(verts_=None) == -3 and call(out_=None) == -3 and call(ws_=None) == -3
    O2 = lib.RenderOut()
    assert call(out_=ctypes.addressof(O2)) == -3                       # a mandatory output missing
    assert call(verts_=None, tl_=5) == -3                              # NULL is reported before a bad shape
    assert call(tl_=5) == -1 and call(nf_=0) == -1 and call(h_=0) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs['im']).all())                          # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    for k in ('im', 'ambient', 'disp', 'flow', 'lit'):
        assert not bool(torch.isnan(outs[k]).any()), k
    assert not bool((outs['tri_id'] == -12345).any())
    # optional outputs absent: the same mandatory outputs
    res = ops.render_track(verts, faces, albedo, R, t, st.K, st.baseline, sc[5], pattern, want_ids=False, workspace=ws)
    assert set(res) == {'im', 'ambient', 'disp', 'flow'}
    for k in res:
        assert torch.equal(res[k], outs[k]), k
    # a ray that hits nothing: disp, flow, im, ambient 0, lit 0, id -1 (one small triangle in the image centre)
    tri = up(np.array([[-0.1, -0.1, 2.0], [0.1, -0.1, 2.0], [0.0, 0.1, 2.0]], dtype=np.float32))
    res = ops.render_track(tri, up(np.array([[0, 1, 2]], dtype=np.int32)), up(np.array([0.5], dtype=np.float32)), R, t, st.K,
                           st.baseline, 0.6, pattern)
    miss = res['tri_id'] < 0
    assert 0 < int((~miss).sum()) < miss.numel() // 20
    assert not bool(res['im'][:, 0][miss].any()) and not bool(res['disp'][:, 0][miss].any()) and not bool(res['lit'][miss].any())
    assert not bool(res['flow'].view(tl, tl, 2, H, W).permute(0, 3, 4, 1, 2)[miss].any()) and bool((res['disp'][:, 0][~miss] > 0).all())
