"""CPU: the numpy restatement of the raycast (tests/raycast_ref.py) held to what the GPU tests lean on - the exemption stays a small
share of every case's pixels and covers every decision the two dtypes take differently - and to the properties of the operation: the
surface it finds lies on the disparities that were integrated, a camera that looks away or sits behind the surface finds none."""
import numpy as np
import pytest

from tests import raycast_inputs as RI
from tests import tsdf_inputs as TI
from tests import tsdf_ref

CAP = 0.005     # exempt pixels per case


@pytest.mark.parametrize('grid', RI.GRIDS, ids=RI.grid_id)
@pytest.mark.parametrize('kind', RI.KINDS)
@pytest.mark.parametrize('shape', RI.SHAPES, ids=TI.shape_id)
def test_the_exemption_is_small_and_covers_the_differences(shape, kind, grid):
    for sv in RI.steps(shape, kind, grid):
        r32, r64, ex = RI.refs(shape, kind, grid, sv)
        m = ~ex
        print(f'step {sv:g}: exempt {100 * ex.mean():.4f} % of {ex.size} pixels, hit {100 * r64["hit"].mean():.1f} %, '
              f'decided differently {int((r32["hit"] != r64["hit"]).sum())}')
        assert ex.mean() <= CAP
        assert np.array_equal(r32['hit'][m], r64['hit'][m]) and np.array_equal(r32['nstar'][m], r64['nstar'][m])
        for k in ('disp', 'value'):
            assert not r64[k][~r64['hit']].any()
        assert not r64['normal'][np.broadcast_to(~r64['hit'][:, None], r64['normal'].shape)].any()
        mh = m & r64['hit']
        if mh.any():
            for k in ('disp', 'value'):
                a32, a64 = r32[k].astype(np.float64)[mh], r64[k][mh]
                assert np.abs(a32 - a64).max() <= tsdf_ref.tolerance(a32, a64)
            assert (r64['disp'][mh] > 0).all()
            ln = np.linalg.norm(r64['normal'], axis=1)[mh]
            assert np.allclose(ln[ln > 0], 1.0, atol=1e-9) and (ln > 0).mean() > 0.99
        # grids of at least 17 points per side: hits and misses in the track's views and in the novel one
        if min(grid) >= 17:
            tl = shape[0]
            assert r64['hit'][:tl].any() and not r64['hit'][:tl].all() and not r64['hit'][tl].all()
            assert r64['hit'][tl].any()


@pytest.mark.parametrize('kind', ['plane', 'bumps', 'holes', 'render'])
@pytest.mark.parametrize('shape', RI.SHAPES, ids=TI.shape_id)
def test_the_surface_lies_on_the_integrated_disparities(shape, kind):
    """ground-truth disparities integrated and cast back at step = voxel: the surface lies within a voxel, so the median relative
    disparity error over the hit pixels is at most voxel / (median depth)"""
    a = TI.make_input(shape, kind)
    tl = shape[0]
    gt = a['disp'].astype(np.float64)
    ok = np.isfinite(gt) & (gt > 0)
    fb = float(np.float32(a['K'][0, 0]) * np.float32(a['baseline']))
    for grid in RI.GRIDS[2:]:
        r64 = RI.refs(shape, kind, grid, 1.0)[1]
        voxel = TI.volume(shape, kind, grid)[1]
        m = r64['hit'][:tl] & ok
        assert m.sum() > 0.2 * ok.sum()
        rel = float(np.median(np.abs(r64['disp'][:tl][m] - gt[m]) / gt[m]))
        bound = voxel / float(np.median(fb / gt[m]))
        print(f'grid {grid}: median |disp - gt| / gt {rel:.3e}, bound {bound:.3e} ({rel / bound:.3f} of it), {int(m.sum())} pixels')
        assert rel <= bound
        # the normals look towards the camera: n . d < 0 with d the ray's direction
        K = a['K'].astype(np.float64)
        v, u = np.indices(shape[1:])
        dc = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u, dtype=np.float64)])
        for f in range(tl):
            dw = np.einsum('jk,jhw->khw', a['R'][f].astype(np.float64), dc)
            dots = (r64['normal'][f] * dw).sum(0)[r64['hit'][f]]
            assert (dots < 0).mean() > 0.99


def _cast(shape, kind, grid, R, t, dtype=np.float64):
    return RI.cast(shape, kind, grid, 1.0, 1, dtype, R=np.asarray(R, dtype=np.float32), t=np.asarray(t, dtype=np.float32))


def test_a_view_that_looks_away_hits_nothing():
    shape, kind, grid = RI.SHAPES[1], 'bumps', RI.GRIDS[2]
    a = TI.make_input(shape, kind)
    turn = np.diag([-1.0, 1.0, -1.0])                       # half a turn about the camera's y axis, the centre stays
    R, t = turn @ a['R'][:1].astype(np.float64), (turn @ a['t'][0].astype(np.float64))[None]
    for dt in (np.float32, np.float64):
        r = _cast(shape, kind, grid, R, t, dt)
        assert not r['hit'].any() and not r['nstar'].any() and not r['disp'].any() and not r['normal'].any() and not r['value'].any()
    assert RI.refs(shape, kind, grid, 1.0)[1]['hit'][0].any()       # (the same camera, not turned, does hit)


@pytest.mark.parametrize('kind', ['plane', 'bumps'])
def test_a_camera_behind_the_surface_hits_nothing(kind):
    """moved forward along its axis to half a voxel behind the surface at the image's centre (the focal length is long: all rays stay
    near the axis), the camera starts inside the band of negative distances: every ray finds a negative sample at once, none has a
    valid non-negative one before it.  Five voxels behind the surface it starts in unobserved space and finds nothing at all."""
    shape, grid = RI.SHAPES[1], RI.GRIDS[3]
    a = TI.make_input(shape, kind)
    voxel = TI.volume(shape, kind, grid)[1]
    fb = float(a['K'][0, 0]) * float(a['baseline'])
    depth = fb / float(a['disp'][0][shape[1] // 2, shape[2] // 2])
    for behind, found in ((0.5, True), (5.0, False)):
        t = a['t'][:1].astype(np.float64) - np.array([0.0, 0.0, depth + behind * voxel])
        r = _cast(shape, kind, grid, a['R'][:1], t)
        print(f'{kind}, {behind:g} voxels behind: {int((r["nstar"] > 0).sum())} of {r["nstar"].size} rays find a negative sample')
        assert not r['hit'].any() and not r['disp'].any() and not r['normal'].any() and not r['value'].any()
        assert (r['nstar'] > 0).all() if found else not r['nstar'].any()
