"""CPU: the numpy restatement of the disparity densification (tests/densify_ref.py) - hand-made cases with the answer written out, the
median against scipy.ndimage.median_filter, what the two stages do to the semi-global matcher's reference output after the speckle
filter - and the file handling of data/presave_sgm.py's --fill / --median / --refilter with the matcher, the filter and the densifier
replaced.  The kernels are pinned to the restatement bit for bit in tests/test_densify_gpu.py."""
import functools
import os

import numpy as np
import pytest

from tests import densify_ref, speckle_ref
from tests.test_speckle_ref_cpu import _dataset, _fake_filter, _fake_matcher, _members, bad_values_image

F = np.float32
FLT_MAX = densify_ref.FLT_MAX


def _run(d, max_gap, min_dirs=1, max_spread=FLT_MAX, median_r=0):
    d = np.asarray(d, dtype=F)
    out, state = densify_ref.disp_densify(d[None] if d.ndim == 2 else d, max_gap, min_dirs, max_spread, median_r)
    return (out[0], state[0]) if d.ndim == 2 else (out, state)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# --------------------------------------------------------------------------------------------------- hand-made cases: the fill
def test_a_walk_reaches_exactly_max_gap():
    row = np.zeros((1, 12), F)
    row[0, 0] = 5
    out, state = _run(row, 4)
    assert np.array_equal(out, [[5, 5, 5, 5, 5, 0, 0, 0, 0, 0, 0, 0]])                  # distance 4 is found, distance 5 is not
    assert np.array_equal(state, [[1, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0]])
    out_t, state_t = _run(row.T, 4)                                                    # the same down a column (an H x 1 image)
    assert np.array_equal(out_t, out.T) and np.array_equal(state_t, state.T)
    # all 8 directions: one valid pixel in the middle reaches the 8 rays of length 3 and nothing else
    d = np.zeros((11, 11), F)
    d[5, 5] = 7
    want = d.copy()
    for dy, dx in densify_ref.DIRECTIONS:
        for s in (1, 2, 3):
            want[5 + s * dy, 5 + s * dx] = 7
    out, state = _run(d, 3)
    assert np.array_equal(out, want) and (want != 0).sum() == 25
    assert np.array_equal(state, np.where(d > 0, 1, np.where(want > 0, 2, 0)))
    assert (_run(d, 32)[0] != 0).sum() == 41                                           # the rays end at the border: 8 x 5 + 1


@pytest.mark.parametrize('dirs', range(1, 9))
def test_min_dirs_on_a_pixel_with_exactly_that_many_directions(dirs):
    d = np.zeros((5, 5), F)
    for dy, dx in densify_ref.DIRECTIONS[:dirs]:
        d[2 + 2 * dy, 2 + 2 * dx] = 5
    for min_dirs in range(1, 9):
        out, state = _run(d, 2, min_dirs)
        assert (out[2, 2], state[2, 2]) == ((5, 2) if min_dirs <= dirs else (0, 0)), (dirs, min_dirs)
        assert np.array_equal(out[d > 0], d[d > 0]) and (state[d > 0] == 1).all()


def test_spread_gate_on_dyadic_values():
    assert np.array_equal(_run([[4, 0, 6]], 1, 2, 2.0)[0], [[4, 4, 6]])                 # a difference equal to max_spread fills ...
    above = np.array([[4, 0, 6 + 2.0 ** -10]], F)
    assert above[0, 2] - F(6) == F(2.0 ** -10)
    out, state = _run(above, 1, 2, 2.0)                                                # ... and 2^-10 above it does not
    assert np.array_equal(out, above) and np.array_equal(state, [[1, 0, 1]])
    assert np.array_equal(_run([[4, 0, 4]], 1, 2, 0.0)[0], [[4, 4, 4]])
    assert np.array_equal(_run([[4, 0, 4 + 2.0 ** -10]], 1, 2, 0.0)[1], [[1, 0, 1]])
    assert np.array_equal(_run([[1, 0, 1e30]], 1, 2, FLT_MAX)[0], np.array([[1, 1, 1e30]], F))    # FLT_MAX: no gate
    assert np.array_equal(_run([[1, 0, 1e30]], 1, 2, 1e29)[1], [[1, 0, 1]])


@pytest.mark.parametrize('ring, want', [
    ([5, 0, 0, 0, 0, 0, 0, 0], 5),                     # m = 1
    ([5, 7, 0, 0, 0, 0, 0, 0], 5),                     # m = 2: the lower of the two
    ([5, 7, 6, 0, 0, 0, 0, 0], 6),                     # m = 3
    ([5, 7, 6, 9, 0, 0, 0, 0], 6),                     # m = 4: v[1]
    ([7, 5, 7, 5, 0, 0, 0, 0], 5),                     # duplicates: 5 5 7 7
    ([7, 5, 7, 5, 7, 0, 0, 0], 7),                     # 5 5 7 7 7
    ([9, 1, 8, 2, 7, 3, 0, 0], 3),                     # m = 6: v[2]
    ([9, 1, 8, 2, 7, 3, 6, 0], 6),                     # m = 7: v[3]
    ([8, 1, 7, 2, 6, 3, 5, 4], 4),                     # m = 8: v[3]
])
def test_fill_takes_the_lower_median(ring, want):
    d = np.zeros((3, 3), F)
    for (dy, dx), v in zip(densify_ref.DIRECTIONS, ring):
        d[1 + dy, 1 + dx] = v
    out, state = _run(d, 1)
    assert out[1, 1] == want and state[1, 1] == 2
    m = sum(v > 0 for v in ring)
    assert m == 8 or _run(d, 1, m + 1)[0][1, 1] == 0


def test_a_filled_pixel_is_not_a_source():
    out, state = _run([[5, 0, 0, 0, 0]], 1)
    assert np.array_equal(out, [[5, 5, 0, 0, 0]]) and np.array_equal(state, [[1, 2, 0, 0, 0]])
    out, state = _run([[5, 0, 0, 0, 9]], 2, 2)                                          # only the middle sees both ends
    assert np.array_equal(out, [[5, 0, 5, 0, 9]]) and np.array_equal(state, [[1, 0, 2, 0, 1]])


def test_images_do_not_see_each_other():
    d = np.zeros((2, 3, 4), F)
    d[0, 0] = 5                                         # the rows below it are holes, and so is the last row of image 0 ...
    d[1, 0] = 9                                         # ... which has the first row of image 1 next to it in memory only
    out, state = _run(d, 2, 1, 0.0)
    assert (out[0] == 5).all() and (out[1] == 9).all()
    assert np.array_equal(state[0], [[1] * 4, [2] * 4, [2] * 4]) and np.array_equal(state[1], state[0])
    e = np.zeros((2, 3, 4), F)
    e[1] = 9
    out, state = _run(e, 32, 1, FLT_MAX, 2)
    assert not out[0].any() and not state[0].any() and (out[1] == 9).all() and (state[1] == 1).all()
    e = e[::-1].copy()
    out, state = _run(e, 32, 1, FLT_MAX, 2)
    assert not out[1].any() and not state[1].any() and (out[0] == 9).all()


def test_values_that_are_not_disparities_come_out_as_plus_zero():
    d = bad_values_image()
    ok = speckle_ref.valid_mask(d)
    assert np.array_equal(densify_ref.valid_mask(d), ok) and (~ok).sum() == 10
    out, state = _run(d, 0)                             # neither stage: the input with the invalid elements as +0.0
    assert np.array_equal(_bits(out), _bits(np.where(ok, F(7), F(0)))) and np.array_equal(state, ok.astype(np.uint8))
    out, state = _run(d, 0, 1, FLT_MAX, 2)              # the median takes them for holes, not for values
    assert np.array_equal(_bits(out), _bits(np.where(ok, F(7), F(0)))) and np.array_equal(state, ok.astype(np.uint8))
    out, state = _run(d, 1, 2, 0.0)                     # every one of them has two 7s beside it
    assert np.array_equal(_bits(out), _bits(np.full(d.shape, 7, F))) and np.array_equal(state, np.where(ok, 1, 2))
    lone = np.array([[np.nan, -np.inf, -0.0, -2, np.inf]], F)
    out, state = _run(lone, 32, 1, FLT_MAX, 2)
    assert (_bits(out) == 0).all() and not state.any()


# --------------------------------------------------------------------------------------------------- hand-made cases: the median
def test_median_over_a_clipped_window():
    d = np.arange(1, 10, dtype=F).reshape(3, 3)
    out, state = _run(d, 0, 1, FLT_MAX, 1)
    # k = 4 at the corners, 6 on the edges, 9 in the middle: v[(k - 1) / 2]
    assert np.array_equal(out, [[2, 3, 3], [4, 5, 5], [5, 6, 6]]) and (state == 1).all()
    assert np.array_equal(_run(d, 0, 1, FLT_MAX, 2)[0], np.full((3, 3), 5, F))          # the image is smaller than the 5 x 5 window
    d[1, 1] = 0
    out, state = _run(d, 0, 1, FLT_MAX, 1)              # the hole stays a hole and is no value: k = 3, 5, 3 / 5, -, 5 / 3, 5, 3
    assert np.array_equal(out, [[2, 3, 3], [4, 0, 6], [7, 7, 8]]) and np.array_equal(state, d > 0)
    dup = np.array([[3, 3, 1, 1, 3, 1]], F)             # 1 x W: k = 2, 3, 3, 3, 3, 2
    assert np.array_equal(_run(dup, 0, 1, FLT_MAX, 1)[0], [[3, 3, 1, 1, 1, 1]])
    assert np.array_equal(_run(dup.T, 0, 1, FLT_MAX, 1)[0], [[3], [3], [1], [1], [1], [1]])
    assert np.array_equal(_run(dup, 0, 1, FLT_MAX, 2)[0], [[3, 1, 3, 1, 1, 1]])          # k = 3, 4, 5, 5, 4, 3


def test_median_reads_the_fill_and_never_its_own_output():
    assert np.array_equal(_run([[1, 9, 2, 8, 3]], 0, 1, FLT_MAX, 1)[0], [[1, 2, 8, 3, 3]])   # (in place the third would be 2)
    out, state = _run([[2, 0, 6]], 1, 1, FLT_MAX, 1)    # the fill gives 2 2 6; over the input the last pixel would stay 6
    assert np.array_equal(out, [[2, 2, 2]]) and np.array_equal(state, [[1, 2, 1]])


def test_single_pixel_images():
    for gap, r in [(0, 0), (32, 0), (0, 2), (32, 2)]:
        out, state = _run(np.full((1, 1), 2.5, F), gap, 1, FLT_MAX, r)
        assert out[0, 0] == F(2.5) and state[0, 0] == 1
        out, state = _run(np.zeros((1, 1), F), gap, 1, FLT_MAX, r)
        assert _bits(out)[0, 0] == 0 and state[0, 0] == 0
    out, state = densify_ref.disp_densify(np.full((2, 1, 1, 1), 4, F))
    assert out.shape == (2, 1, 1, 1) and state.shape == (2, 1, 1) and (out == 4).all()


def _random_map(seed, shape=(3, 40, 56), density=0.6):
    rng = np.random.RandomState(seed)
    d = rng.choice(np.array([5, 6, 7, 20], F), size=shape).astype(F)
    return np.where(rng.rand(*shape) < density, d, F(0)).astype(F)


def test_properties_on_random_maps():
    d = _random_map(0)
    out, state = _run(d, 0)
    assert np.array_equal(_bits(out), _bits(d)) and np.array_equal(state, d > 0)
    for gap, dirs, spread, r in [(16, 6, 2.0, 1), (1, 4, FLT_MAX, 2), (32, 8, 1.0, 0)]:
        out, state = _run(d, gap, dirs, spread, r)
        filled, _ = _run(d, gap, dirs, spread, 0)
        assert np.array_equal(state, np.where(d > 0, 1, np.where(filled > 0, 2, 0))) and (state == 2).any() and (state == 0).any()
        assert np.array_equal(out > 0, state > 0) and (_bits(out)[state == 0] == 0).all()
        assert np.array_equal(filled[d > 0], d[d > 0]) and np.isin(out, [0, 5, 6, 7, 20]).all()
        # the 8 directions map onto themselves under a transposition
        out_t, state_t = _run(d.transpose(0, 2, 1).copy(), gap, dirs, spread, r)
        assert np.array_equal(out_t, out.transpose(0, 2, 1)) and np.array_equal(state_t, state.transpose(0, 2, 1))
        # the images of a batch are independent
        one, one_state = _run(d[1:2], gap, dirs, spread, r)
        assert np.array_equal(one[0], out[1]) and np.array_equal(one_state[0], state[1])


def test_bad_configurations_are_refused():
    d = np.ones((1, 2, 2), F)
    for kw in [dict(max_gap=33), dict(max_gap=-1), dict(min_dirs=0), dict(min_dirs=9), dict(median_r=3), dict(median_r=-1),
               dict(max_spread=-0.5), dict(max_spread=np.nan), dict(max_spread=np.inf)]:
        with pytest.raises(ValueError):
            densify_ref.disp_densify(d, **kw)
    with pytest.raises(ValueError):
        densify_ref.disp_densify(np.ones((2, 2), F))
    with pytest.raises(ValueError):
        densify_ref.disp_densify(np.ones((1, 2, 2, 2), F))


# --------------------------------------------------------------------------------------------------- against scipy
@pytest.mark.parametrize('r', [1, 2])
def test_median_equals_scipy_where_the_window_is_full(r):
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(r)
    d = rng.uniform(1, 60, size=(30, 41)).astype(F)
    out, _ = _run(d, 0, 1, FLT_MAX, r)
    want = ndimage.median_filter(d, size=2 * r + 1, mode='constant')
    assert np.array_equal(out[r:-r, r:-r], want[r:-r, r:-r]) and not np.array_equal(out, d)


# --------------------------------------------------------------------------------------------------- on the matcher's reference output
@functools.lru_cache(maxsize=None)
def _filtered_step_scene(pattern):
    from tests.test_speckle_ref_cpu import _matched_step_scene
    raw, truth = _matched_step_scene(pattern)
    return speckle_ref.speckle_filter(raw[None], 100, 1.0)[0][0], truth


@pytest.mark.parametrize('pattern', ['default', 'real'])
def test_densification_of_the_matchers_output(pattern):
    """tests/sgm_ref.py on the step scene of tests/test_sgm_ref_cpu.py, speckle-filtered with 100 / 1.0, then gap 16, 6 directions,
    spread 2.0 and the 3 x 3 median.  Measured: default valid 0.7365 -> 0.8632, > 1 px 374 -> 44, > 0.5 px 0.1297 -> 0.0240, > 5 px
    0.0015 -> 0.0015, 3 of 3114 filled pixels > 1 px off; real valid 0.8940 -> 0.9152, > 1 px 106 -> 60, > 0.5 px 0.0285 -> 0.0129,
    > 5 px 0.0015 -> 0.0015, 2 of 522."""
    before, truth = _filtered_step_scene(pattern)
    out, state = _run(before, 16, 6, 2.0, 1)
    v0, v1, filled = before != 0, out != 0, state == 2
    e0, e1 = np.abs(before - truth), np.abs(out - truth)
    share0, share1 = float(v0.mean()), float(v1.mean())
    off1_0, off1_1 = int((e0[v0] > 1).sum()), int((e1[v1] > 1).sum())
    half0, half1 = float((e0[v0] > 0.5).mean()), float((e1[v1] > 0.5).mean())
    of5_0, of5_1 = float((e0[v0] > 5).mean()), float((e1[v1] > 5).mean())
    nfilled, filled_off = int(filled.sum()), int((e1[filled] > 1).sum())
    print(f'{pattern}: valid {share0:.4f} -> {share1:.4f}, > 1 px {off1_0} -> {off1_1}, > 0.5 px {half0:.4f} -> {half1:.4f}, '
          f'> 5 px {of5_0:.4f} -> {of5_1:.4f}, filled {nfilled} of {int((~v0).sum())} holes, {filled_off} of them > 1 px off')
    assert np.array_equal(v1, state > 0) and np.array_equal(state == 1, v0)
    if pattern == 'default':
        assert share1 >= 1.1 * share0, (share0, share1)
        assert off1_1 <= 0.25 * off1_0, (off1_0, off1_1)
    assert share1 >= share0, (share0, share1)
    assert off1_1 <= off1_0, (off1_0, off1_1)
    assert half1 <= 0.6 * half0, (half0, half1)
    assert of5_1 <= of5_0 + 0.0005, (of5_0, of5_1)
    assert nfilled > 0 and filled_off <= 0.01 * nfilled, (nfilled, filled_off)


# --------------------------------------------------------------------------------------------------- presave_sgm: file handling
def _fake_densifier(calls):
    def densify(sgm, max_gap, min_dirs, max_spread, median, device='cuda'):
        calls.append((sgm.shape, sgm.dtype, max_gap, min_dirs, max_spread, median))
        hole = sgm == 0
        return np.where(hole, F(1.5), sgm + F(0.25)).astype(F), np.where(hole, 2, 1).astype(np.uint8)      # not idempotent, as the stages
    return densify


def _never(name):
    def f(*a, **k):
        raise AssertionError(f'{name} called')
    return f


def test_defaults_write_what_they_wrote_before(tmp_path, monkeypatch):
    """with --fill and --median off the densifier is never called and frames.npz gets the members - names, order, every byte - that
    rewrite_npz with the matcher's array gives"""
    from depthinspace_amd.data import presave_sgm as P
    from depthinspace_amd.data.trackfiles import rewrite_npz
    root, paths = _dataset(tmp_path)
    monkeypatch.setattr(P, 'match_frames', _fake_matcher)
    monkeypatch.setattr(P, 'filter_speckles', _never('filter_speckles'))
    monkeypatch.setattr(P, 'densify_frames', _never('densify_frames'))
    want = []
    for p in paths:
        q = str(tmp_path / (os.path.basename(p) + '_before.npz'))
        with open(os.path.join(p, 'frames.npz'), 'rb') as f, open(q, 'wb') as g:
            g.write(f.read())
        with np.load(q) as f:
            im = f['im']
        rewrite_npz(q, {'sgm_disp': _fake_matcher(im, None).reshape(im.shape)})
        want.append(_members(q))
    assert P.presave_sgm(root) == 2
    assert [_members(os.path.join(p, 'frames.npz')) for p in paths] == want
    P.main([root, '--fill', '0', '--median', '0'])
    assert [_members(os.path.join(p, 'frames.npz')) for p in paths] == want
    with pytest.raises(ValueError):
        P.presave_sgm(root, refilter=True)               # --refilter without a stage
    for bad in [dict(fill=33), dict(fill=-1), dict(fill=16, fill_dirs=0), dict(fill=16, fill_dirs=9), dict(fill=16, fill_spread=-1.0),
                dict(fill=16, fill_spread=float('nan')), dict(fill=16, fill_spread=float('inf')), dict(median=3), dict(median=-1)]:
        with pytest.raises(ValueError):
            P.presave_sgm(root, **bad)
    assert [_members(os.path.join(p, 'frames.npz')) for p in paths] == want
    res = P.sgm_report(root)                             # no sgm_state: the report has the keys it had
    assert 'filled' not in res and 'of1_filled' not in res and 'valid' in res and 'of1' in res


def test_state_is_written_exactly_when_a_stage_runs(tmp_path, monkeypatch, capsys):
    from depthinspace_amd.data import presave_sgm as P
    root, paths = _dataset(tmp_path, n=3)
    files = [os.path.join(p, 'frames.npz') for p in paths]
    original = [_members(f) for f in files]
    filt, dens = [], []
    monkeypatch.setattr(P, 'match_frames', _fake_matcher)
    monkeypatch.setattr(P, 'filter_speckles', _fake_filter(filt))
    monkeypatch.setattr(P, 'densify_frames', _fake_densifier(dens))

    def strip(k):
        with np.load(files[k]) as f:
            keep = {n: f[n] for n in f.files if n not in ('sgm_disp', 'sgm_state')}
        np.savez(files[k], **keep)

    # the speckle filter alone stores no state
    assert P.presave_sgm(root, speckle=20) == 3 and len(filt) == 3 and dens == []
    for f in files:
        with np.load(f) as z:
            assert 'sgm_disp' in z.files and 'sgm_state' not in z.files
    # fill alone, median alone, all three stages: match, then speckle, then the densifier on what the filter left
    for k, kw, call in [(0, dict(fill=16), (16, 6, 2.0, 0)), (1, dict(median=2), (0, 6, 2.0, 2)),
                        (2, dict(speckle=20, fill=8, fill_dirs=3, fill_spread=0.5, median=1), (8, 3, 0.5, 1))]:
        strip(k)
        del filt[:], dens[:]
        assert P.presave_sgm(root, **kw) == 1
        assert dens == [((4, 1, 32, 48), np.dtype(F)) + call] and len(filt) == (1 if 'speckle' in kw else 0)
        with np.load(files[k]) as z:
            m = _fake_matcher(z['im'], None)
            if 'speckle' in kw:
                m = np.where(m > 20, m, 0).astype(F)
                assert (m == 0).any() and (m != 0).any()
            assert z['sgm_state'].dtype == np.uint8 and z['sgm_state'].shape == (4, 1, 32, 48) and z['sgm_disp'].dtype == F
            assert np.array_equal(z['sgm_state'], np.where(m == 0, 2, 1))
            assert np.array_equal(z['sgm_disp'], np.where(m == 0, F(1.5), m + F(0.25)))
        now = _members(files[k])
        assert [n for n, _, _ in now] == [n for n, _, _ in original[k]] + ['sgm_disp.npy', 'sgm_state.npy']
        assert now[:len(original[k])] == original[k]
    # the command line: the bare flag means a gap of 16
    for argv, call in [(['--fill'], (16, 6, 2.0, 0)), (['--fill', '5', '--fill-dirs', '8', '--fill-spread', '0.25', '--median', '1'],
                                                      (5, 8, 0.25, 1))]:
        strip(0)
        del dens[:]
        P.main([root] + argv)
        assert dens == [((4, 1, 32, 48), np.dtype(F)) + call]
    assert 'left as they are' not in capsys.readouterr().out      # (nothing was refiltered)
    # the report: filled is the share of the valid pixels with state 2, of1_filled the share of those more than 1 px off
    res = P.sgm_report(root)
    valid = filled = off = 0
    for f in files:
        with np.load(f) as z:
            ma = (z['sgm_disp'] != 0) & (z['disp'] > 0)
            fl = ma & (z['sgm_state'] == 2)
            valid, filled, off = valid + int(ma.sum()), filled + int(fl.sum()), off + int((np.abs(z['sgm_disp'] - z['disp'])[fl] > 1).sum())
    assert filled > 0 and res['filled'] == filled / valid and res['of1_filled'] == off / filled
    P.presave_sgm(root, report=True)
    line = capsys.readouterr().out
    assert f'filled {res["filled"]:.4f}' in line and f'of1_filled {res["of1_filled"]:.4f}' in line and 'of5' in line
    strip(1)                                             # one track without state (and without sgm_disp: matched anew, unfiltered)
    assert P.presave_sgm(root) == 1
    assert 'filled' not in P.sgm_report(root)


def test_refilter_skips_final_tracks_and_a_failing_write_keeps_the_file(tmp_path, monkeypatch, capsys):
    from depthinspace_amd.data import presave_sgm as P
    root, paths = _dataset(tmp_path, n=3)
    files = [os.path.join(p, 'frames.npz') for p in paths]
    filt, dens = [], []
    monkeypatch.setattr(P, 'match_frames', _fake_matcher)
    monkeypatch.setattr(P, 'filter_speckles', _fake_filter(filt))
    monkeypatch.setattr(P, 'densify_frames', _fake_densifier(dens))
    assert P.presave_sgm(root) == 3 and filt == [] and dens == []
    raw = [_members(f) for f in files]
    # a failing write leaves the old file in place
    before = [open(f, 'rb').read() for f in files]
    real_savez = np.savez

    def failing_savez(file, **arrays):
        real_savez(file, **{k: v for k, v in arrays.items() if k == 'im'})
        raise OSError('disk full')

    monkeypatch.setattr(P.np, 'savez', failing_savez)
    with pytest.raises(OSError):
        P.presave_sgm(root, fill=16, median=1, refilter=True)
    monkeypatch.setattr(P.np, 'savez', real_savez)
    assert [open(f, 'rb').read() for f in files] == before
    assert all(sorted(os.listdir(p)) == ['flow.npz', 'frames.npz'] for p in paths)
    # track 0 becomes final by a run of its own: --refilter is accepted with --median alone
    with np.load(files[0]) as f:
        keep = {k: f[k] for k in f.files if k != 'sgm_disp'}
    np.savez(files[0], **keep)
    assert P.presave_sgm(root, median=1) == 1
    final0 = open(files[0], 'rb').read()
    stamp0 = os.stat(files[0]).st_mtime_ns
    del filt[:], dens[:]
    capsys.readouterr()
    # --refilter with all stages: the stored arrays of tracks 1 and 2 go through them, track 0 is skipped for every stage
    assert P.presave_sgm(root, speckle=20, fill=16, median=1, refilter=True) == 2
    assert len(filt) == 2 and len(dens) == 2 and dens[0][2:] == (16, 6, 2.0, 1)
    assert '1 tracks' in capsys.readouterr().out
    assert open(files[0], 'rb').read() == final0 and os.stat(files[0]).st_mtime_ns == stamp0
    for k in (1, 2):
        now = _members(files[k])
        assert [n for n, _, _ in now] == [n for n, _, _ in raw[k]] + ['sgm_state.npy']
        assert [(n, b) for n, _, b in now if n not in ('sgm_disp.npy', 'sgm_state.npy')] == [(n, b) for n, _, b in raw[k] if n != 'sgm_disp.npy']
        with np.load(files[k]) as f:
            m = _fake_matcher(f['im'], None)
            m = np.where(m > 20, m, 0).astype(F)
            assert np.array_equal(f['sgm_disp'], np.where(m == 0, F(1.5), m + F(0.25))) and np.array_equal(f['sgm_state'], np.where(m == 0, 2, 1))
    # a second run writes nothing, whatever the stages: every track is final
    after = [open(f, 'rb').read() for f in files]
    stamps = [os.stat(f).st_mtime_ns for f in files]
    del filt[:], dens[:]
    assert P.presave_sgm(root, speckle=20, fill=16, median=1, refilter=True) == 0
    assert '3 tracks' in capsys.readouterr().out
    P.main([root, '--fill', '--median', '1', '--refilter'])
    P.main([root, '--speckle', '20', '--refilter'])
    assert P.presave_sgm(root, fill=16, median=1) == 0
    assert filt == [] and dens == []
    assert [open(f, 'rb').read() for f in files] == after and [os.stat(f).st_mtime_ns for f in files] == stamps
