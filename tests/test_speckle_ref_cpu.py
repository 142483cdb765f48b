"""CPU: the numpy restatement of the speckle filter (tests/speckle_ref.py) - hand-made cases with the answer written out, the partition
against scipy.ndimage.label, what the filter does to the semi-global matcher's reference output - and the file handling of
data/presave_sgm.py's --speckle / --refilter with the matcher and the filter replaced.  The kernels are pinned to the restatement bit for
bit in tests/test_speckle_gpu.py."""
import functools
import os
import zipfile

import numpy as np
import pytest

from tests import sgm_ref, speckle_ref

F = np.float32


def _run(d, max_size, max_diff=1.0):
    d = np.asarray(d, dtype=F)
    out, label, size = speckle_ref.speckle_filter(d[None] if d.ndim == 2 else d, max_size, max_diff)
    return (out[0], label[0], size[0]) if d.ndim == 2 else (out, label, size)


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


# --------------------------------------------------------------------------------------------------- hand-made cases
def test_single_pixel():
    d = np.zeros((3, 3), F)
    d[1, 1] = 5
    out, label, size = _run(d, 0)
    want_label = np.full((3, 3), -1, np.int32)
    want_label[1, 1] = 4
    assert np.array_equal(label, want_label) and np.array_equal(size, (d > 0).astype(np.int32))
    assert np.array_equal(out, d)                       # max_size 0 keeps a component of one pixel
    assert np.array_equal(_run(d, 1)[0], np.zeros((3, 3), F))
    out, label, size = _run(np.full((1, 1), 2.5, F), 0)
    assert out[0, 0] == F(2.5) and label[0, 0] == 0 and size[0, 0] == 1


def test_exactly_max_size_goes_and_one_more_stays():
    d = np.zeros((5, 9), F)
    d[0:2, 0:3] = 10                                    # 6 pixels
    d[1:5, 5] = 20                                      # 7 pixels: an L
    d[4, 5:9] = 20
    out, label, size = _run(d, 6)
    assert (size[0:2, 0:3] == 6).all() and (label[0:2, 0:3] == 0).all()
    assert (size[d == 20] == 7).all() and (label[d == 20] == 1 * 9 + 5).all()
    assert (label[d == 0] == -1).all() and (size[d == 0] == 0).all()
    assert np.array_equal(out, np.where(d == 20, d, 0))
    assert np.array_equal(_run(d, 5)[0], d) and not _run(d, 7)[0].any()


def test_diagonal_pair_is_not_connected():
    out, label, size = _run([[5, 0], [0, 5]], 1)
    assert np.array_equal(label, [[0, -1], [-1, 3]]) and np.array_equal(size, [[1, 0], [0, 1]]) and not out.any()
    # ... and through a shared neighbour it is
    out, label, size = _run([[5, 5], [0, 5]], 2)
    assert np.array_equal(label, [[0, 0], [-1, 0]]) and np.array_equal(size, [[3, 3], [0, 3]]) and np.array_equal(out, [[5, 5], [0, 5]])


def test_ramp_is_one_component_up_to_max_diff():
    i = np.arange(10, dtype=F)
    ramp = (1 + F(0.5) * i)[None]                        # exact in fp32; the ends differ by 4.5
    out, label, size = _run(ramp, 9, 0.5)
    assert (label == 0).all() and (size == 10).all() and np.array_equal(out, ramp)
    steep = (1 + F(0.5 + 2.0 ** -10) * i)[None]          # exact as well: every step is 2^-10 above max_diff
    assert (np.diff(steep[0]) == F(0.5 + 2.0 ** -10)).all()
    out, label, size = _run(steep, 0, 0.5)
    assert np.array_equal(label[0], np.arange(10)) and (size == 1).all() and np.array_equal(out, steep)
    assert not _run(steep, 1, 0.5)[0].any()
    # the same down a column
    out, label, size = _run(ramp.T, 9, 0.5)
    assert (label == 0).all() and (size == 10).all()
    assert (_run(steep.T, 0, 0.5)[2] == 1).all()


BAD_ROW = [7, 7, np.nan, 7, 7, np.inf, 7, -np.inf, 7, -3, 7, 0, 7]


def bad_values_image():
    """two rows: the values that are not disparities stand between regions of 7s; the second row has them one column further"""
    return np.array([BAD_ROW, [7] + BAD_ROW[:-1]], dtype=F)


def test_nan_inf_negative_and_zero_separate_regions():
    d = bad_values_image()
    with np.errstate(invalid='ignore'):
        ok = (d > 0) & (d < np.inf)
    assert np.array_equal(ok[0], [1, 1, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    out, label, size = _run(d, 3, 1.0)
    want_label = np.array([[0, 0, -1, 3, 3, -1, 6, -1, 8, -1, 10, -1, 12],
                           [0, 0, 0, -1, 3, 3, -1, 20, -1, 22, -1, 24, -1]], np.int32)   # the single 7s meet only diagonally
    want_size = np.array([[5, 5, 0, 4, 4, 0, 1, 0, 1, 0, 1, 0, 1],
                          [5, 5, 5, 0, 4, 4, 0, 1, 0, 1, 0, 1, 0]], np.int32)
    assert np.array_equal(label, want_label) and np.array_equal(size, want_size)
    assert np.array_equal(_bits(out), _bits(np.where(want_size > 3, F(7), F(0))))      # every bad value is written as +0.0


def test_components_stay_inside_their_image():
    d = np.zeros((2, 3, 4), F)
    d[0, 2, :] = 5                                      # the last row of image 0 ...
    d[1, 0, :] = 5                                      # ... and the first row of image 1: neighbours in memory only
    d[1, 1, 0] = 5
    out, label, size = _run(d, 4)
    assert (label[0, 2] == 8).all() and (size[0, 2] == 4).all() and not out[0].any()
    assert (label[1][d[1] > 0] == 0).all() and (size[1][d[1] > 0] == 5).all() and np.array_equal(out[1], d[1])


def _random_map(seed, shape=(3, 40, 56)):
    rng = np.random.RandomState(seed)
    return rng.choice(np.array([0, 5, 6, 7, 20], F), size=shape).astype(F)


def test_filter_is_idempotent():
    d = _random_map(0)
    for max_size, max_diff in [(1, 0.0), (7, 1.0), (100, 2.5)]:
        out, label, size = _run(d, max_size, max_diff)
        assert 0 < (out != 0).sum() < (d != 0).sum()
        out2, label2, size2 = _run(out, max_size, max_diff)
        assert np.array_equal(_bits(out2), _bits(out))
        keep = out != 0                                 # what is left is labelled and counted as before
        assert np.array_equal(label2[keep], label[keep]) and np.array_equal(size2[keep], size[keep])
        assert (label2[~keep] == -1).all() and (size2[~keep] == 0).all()


def test_max_size_zero_and_whole_image():
    d = _random_map(1)
    d[0, 0, :5] = [np.nan, np.inf, -1, 0, -np.inf]
    out, label, size = _run(d, 0, 1.0)
    ok = speckle_ref.valid_mask(d)
    assert np.array_equal(_bits(out), _bits(np.where(ok, d, F(0))))
    flat = np.full((1, 6, 7), 3, F)
    assert np.array_equal(_run(flat, 6 * 7 - 1)[0], flat) and not _run(flat, 6 * 7)[0].any() and not _run(d, 40 * 56)[0].any()


def test_bad_configurations_are_refused():
    d = np.ones((1, 2, 2), F)
    for max_size, max_diff in [(-1, 1.0), (1, -0.5), (1, np.nan), (1, np.inf)]:
        with pytest.raises(ValueError):
            speckle_ref.speckle_filter(d, max_size, max_diff)
    with pytest.raises(ValueError):
        speckle_ref.speckle_filter(np.ones((2, 2), F))


# --------------------------------------------------------------------------------------------------- against scipy
@pytest.mark.parametrize('density', [0.4, 0.6, 0.8])
def test_partition_equals_scipy_label(density):
    """with a max_diff above every difference two pixels are linked when both are valid: the components of the mask"""
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(int(density * 10))
    mask = rng.rand(40, 56) < density
    d = np.where(mask, rng.uniform(1, 60, size=mask.shape), 0).astype(F)
    out, label, size = _run(d, 0, 1000.0)
    lab, ncomp = ndimage.label(mask, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    assert ncomp >= 2                                   # (above the percolation threshold few components are left)
    assert (label[~mask] == -1).all() and (size[~mask] == 0).all()
    for k in range(1, ncomp + 1):
        idx = np.flatnonzero(lab == k)                  # ascending: idx[0] is the component's first pixel in row order
        assert (label.flat[idx] == idx[0]).all() and (size.flat[idx] == idx.size).all(), k
    assert len(np.unique(label[mask])) == ncomp


# --------------------------------------------------------------------------------------------------- on the matcher's reference output
@functools.lru_cache(maxsize=None)
def _matched_step_scene(pattern):
    from tests.test_sgm_ref_cpu import step_scene
    im, pat, truth, box = step_scene(pattern)
    res = sgm_ref.sgm_disparity(im[None], pat, ndisp=64)
    return np.asarray(res['disp'], dtype=F)[0], truth


@pytest.mark.parametrize('pattern', ['default', 'real'])
def test_filter_removes_the_matchers_islands(pattern):
    """tests/sgm_ref.py on the step scene of tests/test_sgm_ref_cpu.py, filtered with size 100 and diff 1.0, over all valid pixels: those
    more than 1 px off fall by at least 25 %, the share more than 5 px off does not rise, and at most 3 % of the valid pixels are
    correct ones (<= 1 px off) that the filter removes"""
    raw, truth = _matched_step_scene(pattern)
    out = _run(raw, 100, 1.0)[0]
    v0, v1 = raw != 0, out != 0
    err = np.abs(raw - truth)
    off1_raw, off1_out = int((err[v0] > 1).sum()), int((err[v1] > 1).sum())
    of5_raw, of5_out = float((err[v0] > 5).mean()), float((err[v1] > 5).mean())
    lost = int((v0 & ~v1 & (err <= 1)).sum()) / int(v0.sum())
    print(f'{pattern}: valid {int(v0.sum())} -> {int(v1.sum())}, > 1 px {off1_raw} -> {off1_out}, > 5 px {100 * of5_raw:.2f} % -> '
          f'{100 * of5_out:.2f} %, correct pixels removed {100 * lost:.2f} % of the valid')
    assert np.array_equal(out[v1], raw[v1]) and v1.sum() > 0
    assert off1_out <= 0.75 * off1_raw, (off1_raw, off1_out)
    assert of5_out <= of5_raw, (of5_raw, of5_out)
    assert lost <= 0.03, lost


# --------------------------------------------------------------------------------------------------- presave_sgm: file handling
def _dataset(tmp_path, n=2):
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D
    st = synth.make_settings(32, 48)
    root = str(tmp_path / 'data')
    return root, D.write_synthetic_dataset(root, st, n, seed=5)


def _fake_matcher(im, pattern, ndisp=64, p1=7, p2=60, uniq=5, lr=1, device='cuda'):
    return (im * 40.0 + 1.0).astype(F)


def _fake_filter(calls):
    def filt(sgm, max_size, max_diff=1.0, device='cuda'):
        calls.append((sgm.shape, sgm.dtype, max_size, max_diff))
        return np.where(sgm > max_size, sgm, 0).astype(F)          # idempotent, as the filter is
    return filt


def _members(path):
    """the npz file's members in order: (name, uncompressed bytes)"""
    with zipfile.ZipFile(path) as z:
        return [(i.filename, i.compress_type, z.read(i.filename)) for i in z.infolist()]


def test_speckle_zero_writes_what_it_wrote_before(tmp_path, monkeypatch):
    """the default --speckle 0 never calls the filter, and frames.npz gets the members - names, order, every byte of every array file -
    that the tool's one step before this option existed gives: rewrite_npz with the matcher's array"""
    from depthinspace_amd.data import presave_sgm as P
    from depthinspace_amd.data.trackfiles import rewrite_npz
    root, paths = _dataset(tmp_path)
    monkeypatch.setattr(P, 'match_frames', _fake_matcher)

    def never(*a, **k):
        raise AssertionError('filter_speckles called with --speckle 0')

    monkeypatch.setattr(P, 'filter_speckles', never)
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
    P.main([root, '--speckle', '0'])                     # the command line's default is the same: nothing left to match, nothing filtered
    assert [_members(os.path.join(p, 'frames.npz')) for p in paths] == want
    with pytest.raises(ValueError):
        P.presave_sgm(root, refilter=True)               # --refilter without a size
    for bad in [dict(speckle=-1), dict(speckle=5, speckle_diff=-1.0), dict(speckle=5, speckle_diff=float('nan'))]:
        with pytest.raises(ValueError):
            P.presave_sgm(root, **bad)
    assert [_members(os.path.join(p, 'frames.npz')) for p in paths] == want


def test_speckle_filters_new_arrays_and_refilter_the_stored_ones(tmp_path, monkeypatch):
    from depthinspace_amd.data import presave_sgm as P
    root, paths = _dataset(tmp_path)
    files = [os.path.join(p, 'frames.npz') for p in paths]
    calls = []
    monkeypatch.setattr(P, 'match_frames', _fake_matcher)
    monkeypatch.setattr(P, 'filter_speckles', _fake_filter(calls))
    assert P.presave_sgm(root) == 2 and calls == []
    raw = [_members(f) for f in files]
    with np.load(files[0]) as f:
        keep = {k: f[k] for k in f.files if k != 'sgm_disp'}
    np.savez(files[0], **keep)                          # track 0 has no sgm_disp again
    raw0 = _members(files[0])
    # without --refilter only the new array is filtered; the stored one of track 1 is left alone
    assert P.presave_sgm(root, speckle=20, speckle_diff=0.5) == 1
    assert calls == [((4, 1, 32, 48), np.dtype(F), 20, 0.5)]
    assert _members(files[1]) == raw[1]
    got = dict((n, b) for n, _, b in _members(files[0]))
    assert {k: v for k, v in got.items() if k != 'sgm_disp.npy'} == dict((n, b) for n, _, b in raw0)
    with np.load(files[0]) as f:
        m = _fake_matcher(f['im'], None)
        assert np.array_equal(f['sgm_disp'], np.where(m > 20, m, 0)) and (f['sgm_disp'] == 0).any() and (f['sgm_disp'] != 0).any()
    # --refilter: a failing write leaves the old file in place ...
    before = [open(f, 'rb').read() for f in files]
    real_savez = np.savez

    def failing_savez(file, **arrays):
        real_savez(file, **{k: v for k, v in arrays.items() if k == 'im'})
        raise OSError('disk full')

    monkeypatch.setattr(P.np, 'savez', failing_savez)
    with pytest.raises(OSError):
        P.presave_sgm(root, speckle=20, refilter=True)
    monkeypatch.setattr(P.np, 'savez', real_savez)
    assert [open(f, 'rb').read() for f in files] == before
    assert all(sorted(os.listdir(p)) == ['flow.npz', 'frames.npz'] for p in paths)
    # ... it touches sgm_disp alone, and only where the filter changes it: track 0 is filtered already
    del calls[:]
    assert P.presave_sgm(root, speckle=20, refilter=True) == 1 and len(calls) == 2
    assert open(files[0], 'rb').read() == before[0]
    now = _members(files[1])
    assert [(n, c) for n, c, _ in now] == [(n, c) for n, c, _ in raw[1]]
    assert [(n, b) for n, _, b in now if n != 'sgm_disp.npy'] == [(n, b) for n, _, b in raw[1] if n != 'sgm_disp.npy']
    with np.load(files[1]) as f:
        m = _fake_matcher(f['im'], None)
        assert f['sgm_disp'].dtype == F and np.array_equal(f['sgm_disp'], np.where(m > 20, m, 0).reshape(4, 1, 32, 48))
    # twice gives the same file
    after = [open(f, 'rb').read() for f in files]
    stamps = [os.stat(f).st_mtime_ns for f in files]
    assert P.presave_sgm(root, speckle=20, refilter=True) == 0
    P.main([root, '--speckle', '20', '--refilter'])
    assert [open(f, 'rb').read() for f in files] == after and [os.stat(f).st_mtime_ns for f in files] == stamps
