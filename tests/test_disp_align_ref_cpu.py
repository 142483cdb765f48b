"""CPU: the numpy restatement of the disparity alignment and of the rigid flow (tests/disp_align_ref.py) on rendered tracks - that it
recovers the motion where the flow-based chain of the parent's own restatements (flow_ref.dense_flow -> pose_ref.track_poses) does not,
that its float32 and float64 forms agree, and that the cases the GPU tests use have next to no borderline pixels.

Measured on this file's cases (exact disparities, all 28 ordered pairs): rotation error 1.8e-4 .. 5.0e-3 rad against 1.6e-2 .. 4.5e-2 rad
of the flow-based chain (at least 5 x); end-point error of the rigid flow under the aligned pose 0.016 .. 0.078 px against 0.37 .. 2.10 px
of Horn-Schunck (5.5 .. 88 x) on true flows of 0.36 .. 2.09 px; tolerance(float32, float64) of the poses at most 6.6e-6."""
import numpy as np
import pytest

from tests import disp_align_inputs as DI
from tests import disp_align_ref as DR
from tests import pose_ref


def _off(tl):
    return ~np.eye(tl, dtype=bool)


def test_levels_sizes_and_cameras():
    assert [DR.default_levels(h, w) for _, _, h, w in DI.SHAPES] == [2, 2, 3, 1]
    assert DR.default_levels(512, 432) == 5 and DR.default_levels(8192, 8192) == 6 and DR.default_levels(23, 500) == 1
    assert DR.level_sizes(65, 51, 3) == [(65, 51), (32, 25), (16, 12)]
    c = DR.level_cameras(np.array([[54.4, 0, 23.5], [0, 50.0, 31.5], [0, 0, 1]]), 3)
    assert c[1] == (np.float32(27.2), np.float32(25.0), np.float32(11.5), np.float32(15.5))
    assert c[2][2:] == (np.float32(5.5), np.float32(7.5))          # pixel centres: cell x of level l + 1 covers 2 x and 2 x + 1
    assert DR.schedule(2, (2, 1)) == [(1, True), (0, False), (0, False), (0, False)]
    assert DR.schedule(2, (1, 0)) == [(0, False), (0, False)]     # no pass at the coarsest level: no unit weight


def test_pyramid_keeps_the_nearer_surface_and_maps_stop_at_depth_edges():
    nan, inf = np.nan, np.inf
    p = np.array([[4.0, 4.2, 8.0, 2.0, 1.0],
                  [4.1, 4.3, nan, inf, 1.0],
                  [0.0, -1.0, 5.0, 4.6, 1.0],
                  [nan, -inf, 4.4, 4.5, 1.0],
                  [9.0, 9.0, 9.0, 9.0, 1.0]], np.float32)
    for dt in (np.float32, np.float64):
        d = DR.downsample(p.astype(dt), dt)
        assert d.shape == (2, 2)                                   # the odd row and column are dropped
        want = [[(dt(4.0) + dt(np.float32(4.2)) + dt(np.float32(4.1)) + dt(np.float32(4.3))) / dt(4), dt(8.0)],
                [dt(0.0), (dt(5.0) + dt(np.float32(4.6)) + dt(np.float32(4.5))) / dt(3)]]    # 4.4 < 0.9 * 5: the farther surface
        assert np.array_equal(d, np.array(want, dt))
    ramp = (10 + 0.5 * np.arange(8, dtype=np.float32))[None, :] + np.zeros((6, 1), np.float32)
    ramp[:, 5:] += 4.0                                             # a step of 4.5 between columns 4 and 5: > 2 * 0.15 * D
    ramp[4, 1] = 0.0
    m = DR.target_maps(ramp, np.float32(0.15), np.float32)
    good = m[..., 3] != 0
    assert not good[0].any() and not good[-1].any() and not good[:, 0].any() and not good[:, -1].any()
    assert not good[:, 4].any() and not good[:, 5].any()           # the step
    assert not good[4, 1] and not good[3, 1] and not good[4, 2] and not good[5, 1] and good[2, 1]   # the hole and its neighbours
    assert good[1, 2] and tuple(m[1, 2]) == (11.0, 0.5, 0.0, 1.0) and good[1, 6]
    assert not m[~good].any()


@pytest.mark.parametrize('shape', DI.SHAPES, ids=DI.shape_id)
def test_rigid_flow_of_exact_disparities_is_the_rendered_flow(shape):
    a = DI.make_input(shape, 'exact')
    n, tl, H, W = shape
    flow, vis, _ = DR.rigid_flow(a['disp'], a['R'], a['t'], a['K'], a['baseline'], dtype=np.float64)
    # the renderer's float64 poses are rounded to float32 for the restatement, as for the device: compare under those poses' own flow
    hit = np.repeat(a['disp'] > 0, tl, axis=1).reshape(n, tl * tl, H, W)
    m = a['visible'] & hit
    assert m.mean() > 0.5
    err = np.abs(flow - a['flow']).max(axis=2)[m]
    print(f'max |rigid flow - rendered flow| over {m.sum()} visible pixels: {err.max():.3e} px')
    assert err.max() < 1e-5
    eye = np.arange(tl) * (tl + 1)
    assert not flow[:, eye].any() and not vis[:, eye].any()
    assert not flow[np.broadcast_to((~hit)[:, :, None], flow.shape)].any()
    # A pixel that passes the depth test is visible to the renderer's ray tracer too, but where an occluder lies within tol of the
    # point's disparity: at the lines where two surfaces touch.  (The reverse does not hold: the renderer's flag does not ask for a
    # target inside frame j, and the nearest pixel of a slanted surface can differ by more than tol.)
    off = np.setdiff1d(np.arange(tl * tl), eye)
    v = vis[:, off].astype(bool)
    agree = a['visible'][:, off][v].mean()
    print(f'visible: {v.mean():.3f} of the pixels, of which the renderer sees {agree:.4f}')
    assert v.mean() > 0.25 and agree > 0.9


def _pair_flow(a, b, i, j, R, t):
    """the rigid flow i -> j of track b under the pair pose (R, t): frame i at the origin"""
    disp = a['disp'][b, [i, j]][None]
    Rf = np.stack([np.eye(3), R]).astype(np.float32)[None]
    tf = np.stack([np.zeros(3), t]).astype(np.float32)[None]
    return DR.rigid_flow(disp, Rf, tf, a['K'], a['baseline'], dtype=np.float64)[0][0, 1]


@pytest.mark.parametrize('shape', DI.SHAPES, ids=DI.shape_id)
def test_beats_the_flow_based_chain_on_every_pair(shape):
    a = DI.make_input(shape, 'exact')
    n, tl, H, W = shape
    r64 = DI.refs(shape, 'exact')[1]
    hs_flow, hs_pose = DI.flow_chain(shape)
    assert (r64['stats'][..., 3] == 1).all()
    for b in range(n):
        for i in range(tl):
            for j in range(tl):
                if i == j:
                    continue
                ang = float(DI.rot_angle(r64['state_R'][b, i, j], a['R_pair'][b, i, j]))
                ang_hs = float(DI.rot_angle(hs_pose['state_R'][b, i, j], a['R_pair'][b, i, j]))
                m = a['visible'][b, i * tl + j] & (a['disp'][b, i] > 0)
                truth = a['flow'][b, i * tl + j]
                epe = lambda f: float(np.sqrt(((f - truth) ** 2).sum(0))[m].mean())
                e_al, e_hs = epe(_pair_flow(a, b, i, j, r64['state_R'][b, i, j], r64['state_t'][b, i, j])), epe(hs_flow[b, i * tl + j])
                print(f'track {b} pair {i}{j}: rotation error {ang:.2e} rad (flow chain {ang_hs:.2e}), end-point error {e_al:.3f} px '
                      f'(Horn-Schunck {e_hs:.3f}), true flow {float(np.sqrt((truth ** 2).sum(0))[m].mean()):.2f} px')
                assert ang < ang_hs, (b, i, j, ang, ang_hs)
                assert e_al <= 0.5 * e_hs, (b, i, j, e_al, e_hs)


@pytest.mark.parametrize('case', DI.CASES, ids=DI.case_id)
def test_float32_and_float64_agree_and_no_pixel_is_borderline(case):
    shape, kind = case
    n, tl, H, W = shape
    r32, r64 = DI.refs(shape, kind)
    off = _off(tl)
    assert r64['levels'] == DR.default_levels(H, W) and r64['sums'].shape[0] == sum(DR.DEFAULT_ITERS[:r64['levels']]) + 1
    tol_R, tol_t = pose_ref.tolerance(r32['state_R'], r64['state_R']), pose_ref.tolerance(r32['state_t'], r64['state_t'])
    worst = int(r64['borderline'].max())
    print(f'tolerance R {tol_R:.2e} t {tol_t:.2e}; borderline pixels per pass at most {worst} (float32: {int(r32["borderline"].max())}); '
          f'counts differ by at most {int(np.abs(r32["n_used"] - r64["n_used"]).max())}; used pixels at least {int(r64["n_used"][:, off].min())}')
    assert tol_R < 1e-4 and tol_t < 1e-4
    assert worst <= 4
    assert (np.abs(r32['n_used'] - r64['n_used']) <= r64['borderline'] + r32['borderline']).all()
    assert (r64['stats'][..., 3] == 1).all() and (r32['stats'][..., 3] == 1).all()
    assert r64['n_used'][:, off].min() >= DI.MIN_CORR
    eye = np.arange(tl)
    assert (r64['R_pair'][:, eye, eye] == np.eye(3)).all() and not r64['t_pair'][:, eye, eye].any()
    assert (r64['stats'][:, eye, eye] == np.array([0, 0, 0, 1.0])).all()
    # the statistics are those of the closing pass
    S = r64['sums'][-1]
    assert np.array_equal(r64['stats'][..., 0][:, off], S[..., 29][:, off])
    assert np.allclose(r64['stats'][..., 2][:, off], np.sqrt(S[..., 28][:, off] / S[..., 27][:, off]), rtol=1e-12)


def test_every_kind_of_hole_acts_as_invalid():
    shape = DI.SHAPES[0]
    a = DI.make_input(shape, 'holes')
    assert np.isnan(a['disp']).any() and np.isinf(a['disp']).any() and (a['disp'] < 0).any()
    with np.errstate(invalid='ignore'):
        zeroed = np.where(np.isfinite(a['disp']) & (a['disp'] > 0), a['disp'], np.float32(0))
    r = DI.refs(shape, 'holes')[1]
    z = DR.align_poses(zeroed, a['K'], a['baseline'], min_corr=DI.MIN_CORR)
    for k in ('state_R', 'state_t', 'sums', 'n_used'):
        assert np.array_equal(r[k], z[k]), k
    assert np.isfinite(r['sums']).all() and all(np.isfinite(m).all() for m in r['maps'])
    f1, v1, _ = DR.rigid_flow(a['disp'], a['R'], a['t'], a['K'], a['baseline'])
    f0, v0, _ = DR.rigid_flow(zeroed, a['R'], a['t'], a['K'], a['baseline'])
    assert np.array_equal(f1, f0) and np.array_equal(v1, v0) and np.isfinite(f1).all()
    assert not f1[0, 1][:, zeroed[0, 0] == 0].any()


def test_constant_map_fails_at_a_zero_pivot_and_keeps_the_identity():
    a = DI.make_input(DI.SHAPES[0], 'exact')
    disp = np.full((1, 2, 64, 48), 5.0, np.float32)
    for dt in (np.float32, np.float64):
        r = DR.align_poses(disp, a['K'], a['baseline'], min_corr=DI.MIN_CORR, dtype=dt)
        assert r['n_used'][0, 0, 1, 0] >= DI.MIN_CORR                # enough pixels: it is the pivot that fails
        assert (r['stats'][..., 3] == np.eye(2)).all()
        assert (r['R_pair'] == np.eye(3)).all() and not r['t_pair'].any()


def test_schedule_and_failure_paths():
    shape = DI.SHAPES[0]
    a = DI.make_input(shape, 'exact')
    full = DI.refs(shape, 'exact')[1]
    cheap = DR.align_poses(a['disp'], a['K'], a['baseline'], iters=(4, 4), min_corr=DI.MIN_CORR, margins=False)
    assert cheap['sums'].shape[0] == 9
    assert np.array_equal(cheap['sums'][:4], full['sums'][:4])     # the same passes at the coarsest level
    one = DR.align_poses(a['disp'], a['K'], a['baseline'], levels=1, iters=(10,), min_corr=DI.MIN_CORR, margins=False)
    assert float(DI.rot_angle(one['state_R'][0, 0, 1], a['R_pair'][0, 0, 1])) < 5e-3
    few = DR.align_poses(a['disp'], a['K'], a['baseline'], min_corr=10 ** 6, margins=False)
    assert (few['stats'][..., 3] == np.eye(2)).all() and (few['R_pair'] == np.eye(3)).all()
    assert few['stats'][0, 0, 1, 0] > 0                             # the closing pass still measures
