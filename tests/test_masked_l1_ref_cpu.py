"""CPU: the numpy restatement of the masked multi-scale pseudo-GT term (tests/masked_l1_ref.py) against a triple-loop brute force, on
(planes, H, W) = (3, 5, 7) for every erosion radius and the hole layouts the GPU tests reuse."""
import numpy as np
import pytest

from tests import masked_l1_ref as R

P, H, W = 3, 5, 7


def _inputs(seed, n=4):
    rng = np.random.RandomState(seed)
    t = (np.abs(R.dyadic(rng, (P, 1, H, W))) + np.float32(1 / 64)).astype(np.float32)
    outs = [R.dyadic(rng, (P, 1, H, W)) for _ in range(n)]
    outs[0][0, 0, 2, 3] = t[0, 0, 2, 3]          # a zero difference: sign(0) = 0
    gs = [1.0, 0.5, 0.25, 3.0][:n]
    return outs, t, gs


def _same(a, b):
    va, ga, na = a
    vb, gb, nb = b
    assert na == nb
    for x, y in zip(va, vb):
        assert x.dtype == np.float32 and np.float32(x).tobytes() == np.float32(y).tobytes(), (x, y)
    for x, y in zip(ga, gb):
        assert x.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize('r', [0, 1, 2, 3])
@pytest.mark.parametrize('layout', ['none', 'corners', 'last_row_plane0', 'all_hole_plane', 'all_holes'])
def test_restatement_matches_brute_force(layout, r):
    outs, t, gs = _inputs(3 + r)
    if layout != 'none':
        t = R.punch(t, R.hole_layouts(P, H, W)[layout])
    got = R.masked_l1_multi(outs, t, r, gs)
    _same(got, R.brute_force(outs, t, r, gs))
    if layout == 'all_holes':
        assert got[2] == 0 and all(v == 0 for v in got[0]) and all(not g.any() for g in got[1])
    if layout == 'none':
        assert got[2] == P * H * W                # pixels outside the image do not invalidate
        assert got[1][0][0, 0, 2, 3] == 0
    if layout == 'last_row_plane0':
        v = R.valid_mask(t, r)
        assert v[1].all() and v[2].all()          # a window never reads another plane
        assert not v[0, H - 1 - r:].any() and v[0, :H - 1 - r].all()
    if layout == 'all_hole_plane':
        v = R.valid_mask(t, r)
        assert not v[1].any() and v[0].all() and v[2].all()


@pytest.mark.parametrize('r', [0, 1, 3])
def test_nan_target_is_a_hole_and_masking_is_a_select(r):
    outs, t, gs = _inputs(11)
    t[1, 0, 2, 2] = np.nan                        # not > 0: a hole
    t[2, 0, 4, 6] = 0.0
    outs[1][2, 0, 4, 6] = np.inf                  # an inf estimate under a hole
    outs[2][1, 0, 2, 2] = np.nan
    t[0, 0, 0, 0] = -3.0                          # negative: a hole as well
    got = R.masked_l1_multi(outs, t, r, gs)
    _same(got, R.brute_force(outs, t, r, gs))
    assert all(np.isfinite(v) for v in got[0]) and all(np.isfinite(g).all() for g in got[1])
    v = R.valid_mask(t, r)
    assert not v[1, 2, 2] and not v[2, 4, 6] and not v[0, 0, 0]
    assert int(v.sum()) == got[2] and 0 < got[2] < P * H * W
    if r == 1:
        assert not v[1, 1:4, 1:4].any() and v[1, 0, 0] and not v[2, 3:, 5:].any()


def test_one_count_serves_all_scales_and_views():
    outs, t, gs = _inputs(5)
    t = R.punch(t, R.hole_layouts(P, H, W)['corners'])
    one = [R.masked_l1_multi([o], t, 1, [g]) for o, g in zip(outs, gs)]
    allv = R.masked_l1_multi(outs, t, 1, gs)
    for k in range(4):
        assert one[k][0][0] == allv[0][k] and np.array_equal(one[k][1][0], allv[1][k])
    # (tl, bs, 1, H, W) views: the same planes
    five = R.masked_l1_multi([o.reshape(3, 1, 1, H, W) for o in outs], t.reshape(3, 1, 1, H, W), 1, gs)
    assert [v for v in five[0]] == [v for v in allv[0]] and five[1][0].shape == (3, 1, 1, H, W)
