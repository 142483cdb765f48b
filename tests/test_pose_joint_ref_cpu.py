"""CPU: the numpy restatement of the joint pose refinement (tests/pose_joint_ref.py) against its own objective, against the truth of the
synthetic inputs and against the pairwise estimate it starts from - what the GPU test (tests/test_pose_joint_gpu.py) then holds the
kernels to - and the part of data/presave_pose.py that chains a starting point.

Nothing here is a stored number: errors are measured against the poses the inputs were made with, and bounds come from the distance
between the float32 and the float64 restatement (pose_ref.tolerance), from the pairwise estimate of the same quantity, or are derived
where they are used."""
import numpy as np
import pytest

from tests import pose_inputs as PI
from tests import pose_joint_inputs as JI
from tests import pose_joint_ref as JR
from tests import pose_ref

BIG = JI.SHAPES[3]                                  # 1 x 4 x 64 x 96: all 12 pairs


def _perturb(R, t, xi):
    """a left perturbation xi (6 (tl - 1)) of the frames 1 .. tl - 1"""
    R, t = R.copy(), t.copy()
    for f in range(1, len(R)):
        R[f], t[f] = JR.exp_update(xi[6 * (f - 1):6 * f], R[f], t[f])
    return R, t


@pytest.mark.parametrize('case', [((1, 3, 19, 37), 'bumps'), (BIG, 'render')], ids=JI.case_id)
def test_the_right_hand_side_is_the_gradient_of_the_objective(case):
    """2 b = the derivative of sum r2 g (over the contributing pairs) under a left perturbation of every frame but frame 0, in float64:
    this pins the signs and the block order of the adjoint.  (The weight of iterated least squares for the objective r2 g is g g.)
    The central difference D(h) = (F(h) - F(-h)) / 2h differs from the derivative by
      truncation  c h^2 + O(h^4); D(2h) - D(h) = 3 c h^2 + O(h^4) measures it: |D(2h) - D(h)| / 3, allowed twice for the O(h^4) terms;
      rounding    the residuals are formed from pixel coordinates up to max(H, W) and carry delta <= 16 2^-52 max(H, W) each, r2 then
                  2 |e| delta + delta^2 and F over n pixels at most dF = 2 sqrt(n F) delta + n delta^2 (Cauchy-Schwarz; the bound of
                  tests/test_pose_ref_cpu.py): two such values over 2h give dF / h;
    and b itself, a sum of n float64 terms, is taken to 16 2^-52 sqrt(n) of its largest component."""
    shape, kind = case
    n_, tl, H, W = shape
    assert (n_, tl, H, W) in ((1, 3, 19, 37), (1, 4, 64, 96))
    a = JI.make_input(shape, kind)
    R0, t0, _ = JI.init(shape, kind, 'perturbed')
    trk = JR.Track(a['disp'][0], a['flow'][0], a['K'], a['baseline'], 1.0, np.ones((tl, tl), bool), np.float64)
    R, t = R0[0].astype(np.float64), t0[0].astype(np.float64)
    sums, ads, contrib, F0 = trk.pass_(R, t, JI.MIN_CORR)
    assert len(contrib) == tl * (tl - 1)
    A, b = JR.assemble(tl, sums, ads, contrib)
    npix = sum(sums[p][29] for p in contrib)
    m = 6 * (tl - 1)
    h = 1e-5

    def F(xi):
        s_, a_, c_, cost = trk.pass_(*_perturb(R, t, xi), JI.MIN_CORR)
        assert c_ == contrib and all(s_[p][29] == sums[p][29] for p in contrib)      # the same pixels: the objective is smooth here
        return cost

    delta = 16 * 2.0 ** -52 * max(H, W)
    dF = 2 * np.sqrt(npix * F0) * delta + npix * delta ** 2
    worst = 0.0
    for k in range(m):
        e = np.zeros(m)
        e[k] = 1.0
        D1 = (F(h * e) - F(-h * e)) / (2 * h)
        D2 = (F(2 * h * e) - F(-2 * h * e)) / (4 * h)
        allowed = 2 * abs(D2 - D1) / 3 + dF / h + 16 * 2.0 ** -52 * np.sqrt(npix) * float(np.abs(2 * b).max())
        print(f'component {k}: 2 b {2 * b[k]:.9e}, central difference {D1:.9e}, difference {abs(D1 - 2 * b[k]):.3e}, allowed {allowed:.3e}')
        assert abs(D1 - 2 * b[k]) <= allowed
        worst = max(worst, allowed / abs(2 * b[k]))
    assert worst < 1e-3                              # the check can tell a wrong sign or a swapped block from a right one
    # and the matrix is the symmetric Gauss-Newton one: a step along -A^-1 b descends
    assert np.array_equal(A, A.T) or float(np.abs(A - A.T).max()) <= 1e-12 * float(np.abs(A).max())
    d = JR.solve(A, b, 0.0)
    assert d is not None and F(1e-3 * d) < F0


@pytest.mark.parametrize('shape', [s for s in JI.SHAPES if s != JI.SHAPES[0]], ids=PI.shape_id)
def test_exact_planes_are_reached_from_the_perturbed_truth(shape):
    a = JI.make_input(shape, 'plane')
    for pi in (0, 2):
        p32, p64 = PI.refs(shape, 'plane', pi)
        r64 = JI.refs(shape, 'plane', pi, 'perturbed')[1]
        assert np.all(r64['track_stats'][:, 3] == 1) and np.all(r64['steps'] == JI.PARAMS[pi][0])
        start = JI.pose_error(*JI.init(shape, 'plane', 'perturbed')[:2], a)
        err = JI.pose_error(r64['state_R'], r64['state_t'], a)
        for k, e, s in (('R_pair', err[0], start[0]), ('t_pair', err[1], start[1])):
            allowed = pose_ref.tolerance(p32[k], p64[k])       # what the pairwise restatement is held to on the same input
            print(f'params {pi} {k}: max |joint64 - truth| {e:.3e} (start {s:.3e}), allowed {allowed:.3e}')
            assert e <= allowed and s > 1e-3


PLAIN = [k for k in PI.INPUTS if k != 'no_overlap']


@pytest.mark.parametrize('kind', PLAIN)
def test_joint_is_not_worse_than_pairwise(kind):
    """on plane and holes both errors sit at the float32 floor of the truth"""
    a = JI.make_input(BIG, kind)
    p32, p64 = PI.refs(BIG, kind, 0)
    r64 = JI.refs(BIG, kind, 0)[1]
    pw, jt = JI.pose_error(*JI.init(BIG, kind)[:2], a), JI.pose_error(r64['state_R'], r64['state_t'], a)
    for k, e_pw, e_jt in (('R_pair', pw[0], jt[0]), ('t_pair', pw[1], jt[1])):
        allowed = e_pw + pose_ref.tolerance(p32[k], p64[k])
        print(f'{kind} {k}: pairwise {e_pw:.3e}, joint {e_jt:.3e}, allowed {allowed:.3e}')
        assert e_jt <= allowed
    if kind in ('plane', 'holes'):
        assert max(pw[0], jt[0]) < 16 * 2.0 ** -23


@pytest.mark.parametrize('base', JI.BROKEN_BASES)
def test_joint_halves_the_error_of_a_broken_pair(base):
    """two pairs with frame 0 are broken and still report status 1: the composed pairwise poses carry the wrong pair, the joint ones
    are held by the ten others.  The cap of a half is a condition (the worst ratio measured is 0.27), not a tolerance."""
    kind = base + '+broken'
    a = JI.make_input(BIG, kind)
    assert np.all(JI.pairwise(BIG, kind)['stats'][..., 3] == 1)
    r64 = JI.refs(BIG, kind, 0)[1]
    pw, jt = JI.pose_error(*JI.init(BIG, kind)[:2], a), JI.pose_error(r64['state_R'], r64['state_t'], a)
    clean = JI.pose_error(*JI.init(BIG, base)[:2], a)
    print(f'{kind}: pairwise R {pw[0]:.3e} t {pw[1]:.3e}, joint R {jt[0]:.3e} t {jt[1]:.3e}, ratios {jt[0] / pw[0]:.3f} {jt[1] / pw[1]:.3f}')
    assert pw[0] > 2 * clean[0] and pw[1] > 2 * clean[1]       # the pairs are broken
    assert jt[0] <= 0.5 * pw[0] and jt[1] <= 0.5 * pw[1]


def _conditions(r32, r64):
    assert np.array_equal(r32['pair_stats'][..., 0], r64['pair_stats'][..., 0]) and np.array_equal(r32['pair_stats'][..., 3], r64['pair_stats'][..., 3])
    for k in (0, 1, 3):
        assert np.array_equal(r32['track_stats'][..., k], r64['track_stats'][..., k])
    assert np.array_equal(r32['steps'], r64['steps'])
    for k in ('R', 't'):
        allowed = pose_ref.tolerance(r32[k], r64[k])
        print(f'{k}: tolerance {allowed:.3e}, max |ref32 - ref64| {float(np.abs(r32[k] - r64[k]).max()):.3e}')
        assert allowed <= 1e-4
    assert all(np.all(np.isfinite(r64[k])) for k in ('R', 't', 'pair_stats', 'track_stats'))


@pytest.mark.parametrize('case', JI.CASES, ids=JI.case_id)
def test_conditions_the_gpu_test_rests_on(case):
    """the GPU test compares counts, flags and status exactly with the float32 restatement and floats with the float64 one inside
    pose_ref.tolerance: that only means something while the two restatements agree on the former and the tolerance stays small"""
    _conditions(*JI.refs(*case, 0))


def test_conditions_of_the_other_gpu_cases():
    for case in ((JI.SHAPES[2], 'noise'), (BIG, 'contam+broken')):
        for pi in (1, 2):
            _conditions(*JI.refs(*case, pi))
    for case in ((BIG, 'render'), (JI.SHAPES[2], 'bumps')):
        _conditions(*JI.refs(*case, 0, 'perturbed'))
    _conditions(*JI.refs(BIG, 'noise+broken', 0, masked=True))


def _frame_2_unused(tl=4):
    use = np.ones((1, tl, tl), np.uint8)
    use[:, 2, :] = 0
    use[:, :, 2] = 0
    return use


def _refine(a, R0, t0, use, dt=np.float64, flow=None):
    iters, scale, damping = JI.PARAMS[0]
    return JR.refine_track_poses(a['disp'], a['flow'] if flow is None else flow, a['K'], a['baseline'], R0, t0, use, iters, scale, damping,
                                 JI.MIN_CORR, dtype=dt)


def test_failed_tracks_keep_the_init():
    for shape, kind in ((JI.SHAPES[0], 'plane'), (JI.SHAPES[0], 'noise'), (JI.SHAPES[1], 'no_overlap'), (BIG, 'no_overlap')):
        R0, t0, _ = JI.init(shape, kind)
        for r in JI.refs(shape, kind, 0):
            assert np.all(r['track_stats'][:, [0, 1, 3]] == 0) and np.all(r['steps'] == 0) and np.all(r['pair_stats'][..., 3][:, ~np.eye(shape[1], dtype=bool)] == 0)
            assert np.array_equal(r['R'].astype(np.float32), R0) and np.array_equal(r['t'].astype(np.float32), t0)
            if kind == 'no_overlap':
                assert np.all(r['pair_stats'][..., :3] == 0) and np.all(r['track_stats'] == 0)
    # every pair that is used contributes, yet no pair touches frame 2: its pivot is zero
    a = JI.make_input(BIG, 'noise')
    R0, t0, _ = JI.init(BIG, 'noise')
    for dt in (np.float32, np.float64):
        r = _refine(a, R0, t0, _frame_2_unused(), dt)
        assert r['track_stats'][0, 3] == 0 and r['track_stats'][0, 0] == 6 and r['steps'][0] == 0
        assert np.array_equal(r['R'].astype(np.float32), R0) and np.array_equal(r['t'].astype(np.float32), t0)
        assert np.all(r['pair_stats'][0, 2, [0, 1, 3]] == 0) and np.all(r['pair_stats'][0, [0, 1, 3], 2] == 0)
        assert np.all(r['pair_stats'][0, np.eye(4, dtype=bool)] == np.array([0, 0, 0, 1]))


def test_the_flows_of_unused_pairs_are_not_read():
    a, broken = JI.make_input(BIG, 'noise'), JI.make_input(BIG, 'noise+broken')
    R0, t0, _ = JI.init(BIG, 'noise')
    use = np.ones((1, 4, 4), np.uint8)
    for (i, j) in JI.BROKEN_PAIRS:
        use[0, i, j] = 0
    want = _refine(a, R0, t0, use)
    nans = a['flow'].copy()
    for (i, j) in JI.BROKEN_PAIRS:
        nans[:, i * 4 + j] = np.nan
    for flow in (broken['flow'], nans):
        got = _refine(a, R0, t0, use, flow=flow)
        for k in ('R', 't', 'pair_stats', 'track_stats'):
            assert np.array_equal(got[k], want[k]), k
    assert want['track_stats'][0, 0] == 10 and want['track_stats'][0, 3] == 1
    assert np.all(want['pair_stats'][0, 0, 2] == 0) and np.all(want['pair_stats'][0, 2, 0] == 0)
    every = JI.refs(BIG, 'noise', 0)[1]
    assert not np.array_equal(every['R'], want['R'])            # (the mask is not ignored)


# ------------------------------------------------------------------------------------------------ data/presave_pose.py
def test_chain_track_walks_breadth_first_from_frame_0():
    from depthinspace_amd.data import presave_pose as PP
    from tests.test_pose_ref_cpu import _hand_made_track
    R, t, Rp, tp = _hand_made_track()
    tl = len(R)
    ok = np.ones((tl, tl), bool)
    for mask in (ok, np.triu(ok), np.tril(ok)):                 # wherever compose_track has an answer, the chain gives the same one
        a, b = PP.compose_track(Rp, tp, mask), PP.chain_track(Rp, tp, mask)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and b[0].dtype == np.float32
    # frame 2 has lost both pairs with frame 0: compose_track gives up, the chain goes 0 -> 1 -> 2 (frame 1 is reached first)
    ok = np.ones((tl, tl), bool)
    ok[0, 2] = ok[2, 0] = False
    bad_R, bad_t = Rp.copy(), tp.copy()
    bad_R[0, 2] = bad_R[2, 0] = np.nan
    assert PP.compose_track(bad_R, bad_t, ok) is None
    got = PP.chain_track(bad_R, bad_t, ok)
    assert np.allclose(got[0], R, atol=1e-6) and np.allclose(got[1], t, atol=1e-6)
    marked = bad_R.copy()
    marked[3, 2] = marked[2, 3] = np.nan                          # frame 3 is not asked: frame 1 has an answer and comes first
    assert np.array_equal(PP.chain_track(marked, bad_t, ok)[0], got[0])
    ok[1, 2] = False                                            # the inverse of (2, 1) takes its place
    bad_R[1, 2] = np.nan
    got = PP.chain_track(bad_R, bad_t, ok)
    assert np.allclose(got[0], R, atol=1e-6) and np.allclose(got[1], t, atol=1e-6)
    ok[2, :] = ok[:, 2] = False                                 # out of reach
    assert PP.chain_track(bad_R, bad_t, ok) is None
