"""CPU: the numpy restatement of the semi-global matcher (tests/sgm_ref.py) - its quality on inputs with known disparities, its edge
semantics - and the file handling of data/presave_sgm.py with the matcher replaced.  The quality caps are conditions on the reference
(a restatement that misses them differs from the algorithm in include/dis_hip.h); the kernels are pinned to it bit for bit in
tests/test_sgm_gpu.py."""
import os

import numpy as np
import pytest

from tests import sgm_ref


def _quality(res, truth, umin):
    """valid fraction and, of the valid pixels, the fraction more than 1 px off, over the columns u >= umin"""
    ok = res['valid'][..., umin:]
    err = np.abs(res['disp'] - truth)[..., umin:]
    return float(ok.mean()), float((err[ok] > 1).mean())


@pytest.mark.parametrize('pattern', ['default', 'real'])
@pytest.mark.parametrize('scene', ['plane', 'bumps'])
def test_reference_on_synthetic_frames(pattern, scene):
    """Input A: synth.make_batch frames at 96 x 160; valid >= 0.80, at most 3 % of the valid pixels off by more than 1 px"""
    from depthinspace_amd import synth
    st = synth.make_settings(96, 160, pattern=pattern)
    b = synth.make_batch(st, 1, tl=2, seed=7, scene=scene, with_flow=False, with_primary=False)
    im, truth = b['im0'][0, :, 0], b['disp0'][0, :, 0]
    res = sgm_ref.sgm_disparity(im, st.pattern[..., 0], ndisp=64)
    valid, bad = _quality(res, truth, int(np.ceil(truth.max())) + 5)
    print(f'{pattern} {scene}: valid {valid:.3f}, > 1 px {100 * bad:.2f} %')
    assert valid >= 0.80 and bad <= 0.03, (valid, bad)
    assert (res['disp'][~res['valid']] == 0).all()


def step_scene(pattern):
    """Input B: 128 x 192, a slanted background with a nearer slanted box in front of it"""
    from depthinspace_amd import synth
    H, W = 128, 192
    pat = synth.make_settings(H, W, pattern=pattern).pattern[..., 0].astype(np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    box = (u > 70) & (u < 150) & (v > 30) & (v < 100)
    disp = np.where(box, 30 + 0.03 * (v - 30), 6 + 0.02 * u + 0.01 * v)
    amb = 0.5 + 0.25 * np.sin(0.05 * u) * np.cos(0.04 * v)
    noise = np.random.RandomState(3).normal(0, 1.0 / 255, size=(H, W))
    im = np.clip(0.6 * synth._bilinear_border(pat, u - disp, v) + 0.4 * amb + noise, 0, 1)
    return im.astype(np.float32), pat.astype(np.float32), disp.astype(np.float32), box


@pytest.mark.parametrize('pattern', ['default', 'real'])
def test_reference_on_step_scene(pattern):
    """Input B; valid >= 0.70, at most 4 % of the valid pixels off by more than 1 px, valid inside the box >= 0.60 (u >= 40)"""
    im, pat, truth, box = step_scene(pattern)
    res = sgm_ref.sgm_disparity(im[None], pat, ndisp=64)
    valid, bad = _quality(res, truth[None], 40)
    inbox = float(res['valid'][0][box].mean())
    print(f'{pattern}: valid {valid:.3f}, > 1 px {100 * bad:.2f} %, valid in the box {inbox:.3f}')
    assert valid >= 0.70 and bad <= 0.04 and inbox >= 0.60, (valid, bad, inbox)


def test_constant_image_is_all_invalid():
    """a constant image has the census word 0 everywhere; against a constant pattern every in-range candidate costs 0 on every path,
    the lowest one wins the tie, d0 = 0, and d0 >= 1 fails: nothing is valid"""
    res = sgm_ref.sgm_disparity(np.full((1, 20, 70), 0.5, np.float32), np.full((20, 70), 0.25, np.float32), ndisp=64)
    assert (res['census'] == 0).all()
    assert (res['d_int'] == 0).all() and not res['valid'].any() and (res['disp'] == 0).all()
    # against a textured pattern the image's census is still 0 and column 0, where only d = 0 is in range, still has d0 = 0
    pat = np.random.RandomState(0).rand(20, 70).astype(np.float32)
    res = sgm_ref.sgm_disparity(np.full((1, 20, 70), 0.5, np.float32), pat, ndisp=64)
    assert (res['census'][0] == 0).all() and (res['d_int'][0, :, 0] == 0).all() and not res['valid'][0, :, 0].any()


def test_narrower_than_the_candidate_range():
    """W < ndisp: candidates d > u cost 64 on every path and never win; the right view's search stops at the image edge"""
    rng = np.random.RandomState(1)
    pat = rng.rand(24, 40).astype(np.float32)
    im = np.stack([np.roll(pat, 5, axis=1), rng.rand(24, 40).astype(np.float32)])
    res = sgm_ref.sgm_disparity(im, pat, ndisp=64)
    u = np.broadcast_to(np.arange(40)[None, None, :], res['d_int'].shape)
    assert res['vol'].min() >= 0 and res['vol'].max() <= 8 * (64 + 60)
    assert (res['vol'][:, :, 0, 1:] >= 8 * 64).all()               # column 0: only d = 0 is in range
    assert (res['d_int'][res['valid']] <= u[res['valid']]).all()
    assert (res['disp'][res['valid']] >= 0.5).all() and (res['disp'] < 40).all()
    inner = res['d_int'][0, 4:-4, 12:-5]
    assert (inner == 5).mean() > 0.95                              # the shifted copy is found


def test_lowest_candidate_wins_ties():
    S = np.full((1, 1, 70, 64), 100, np.int64)
    S[..., 7] = 3
    S[..., 20] = 3
    disp, d0, ok = sgm_ref.winner(S, uniq=0, lr=100)
    assert (d0 == 7).all()
    assert not ok.any()                                            # s2 == s0: the strict uniqueness test fails even at uniq = 0
    S[..., 20] = 4
    S[..., 6] = 9
    S[..., 8] = 5
    disp, d0, ok = sgm_ref.winner(S, uniq=0, lr=100)
    assert ok[0, 0, 7:].all() and not ok[0, 0, :7].any()           # u - d0 >= 0
    want = np.float32(7) + np.float32(9 - 5) / (np.float32(2) * np.float32(9 + 5 - 6))
    assert (disp[0, 0, 7:] == want).all() and (disp[0, 0, :7] == 0).all()
    # the right view breaks its ties towards the lowest d as well: with every S equal, dR = 0 and lr = 0 rejects d0 = 7 ... never reached,
    # the argmin itself is 0 and d0 >= 1 fails
    disp, d0, ok = sgm_ref.winner(np.full((1, 2, 70, 64), 50, np.int64), uniq=0, lr=0)
    assert (d0 == 0).all() and not ok.any()


# --------------------------------------------------------------------------------------------------- presave_sgm: file handling
def _dataset(tmp_path, n=2):
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D
    st = synth.make_settings(32, 48)
    root = str(tmp_path / 'data')
    return root, st, D.write_synthetic_dataset(root, st, n, seed=5)


def _fake_matcher(calls):
    def match(im, pattern, ndisp=64, p1=7, p2=60, uniq=5, lr=1, device='cuda'):
        calls.append((im.shape, pattern.shape, ndisp, p1, p2, uniq, lr))
        return (im * 40.0 + 1.0).astype(np.float32)
    return match


def test_presave_rewrites_frames_incrementally(tmp_path, monkeypatch):
    from depthinspace_amd.data import presave_sgm as P, dataset as D, packed
    root, st, paths = _dataset(tmp_path)
    before = [{k: v.copy() for k, v in np.load(os.path.join(p, 'frames.npz')).items()} for p in paths]
    calls = []
    monkeypatch.setattr(P, 'match_frames', _fake_matcher(calls))
    assert P.presave_sgm(root, ndisp=128, p1=3, p2=50, uniq=9, lr=2) == 2
    assert calls == [((4, 1, 32, 48), (32, 48), 128, 3, 50, 9, 2)] * 2
    for p, old in zip(paths, before):
        assert sorted(os.listdir(p)) == ['flow.npz', 'frames.npz']              # no temporary file is left
        with np.load(os.path.join(p, 'frames.npz')) as f:
            assert sorted(f.files) == sorted(list(old) + ['sgm_disp'])
            for k, v in old.items():
                assert f[k].dtype == v.dtype and f[k].shape == v.shape and f[k].tobytes() == v.tobytes(), k
            assert f['sgm_disp'].dtype == np.float32 and f['sgm_disp'].shape == (4, 1, 32, 48)
            assert np.array_equal(f['sgm_disp'], old['im'] * np.float32(40.0) + np.float32(1.0))
    # incremental: a track that has the array is left alone, bit for bit and untouched on disk
    stamp = [os.stat(os.path.join(p, 'frames.npz')).st_mtime_ns for p in paths]
    with np.load(os.path.join(paths[1], 'frames.npz')) as f:
        keep = {k: f[k] for k in f.files if k != 'sgm_disp'}
    np.savez(os.path.join(paths[1], 'frames.npz'), **keep)
    del calls[:]
    assert P.presave_sgm(root) == 1 and len(calls) == 1
    assert os.stat(os.path.join(paths[0], 'frames.npz')).st_mtime_ns == stamp[0]
    # the `real` reader returns the array, and the packer sees it
    ds = D.TrackNpzDataset(root, paths, track_length=4, train=False, data_type='real')
    s = ds[0]
    assert tuple(s['sgm_disp'].shape) == (4, 1, 32, 48) and np.array_equal(s['sgm_disp'].numpy(), s['im0'].numpy() * np.float32(40.0) + np.float32(1.0))
    assert P.presave_sgm(root, pack=True) == 0
    assert 'sgm_disp' in packed.read_meta(root)['frames_fields']
    hw = 32 * 48
    assert os.path.getsize(os.path.join(paths[0], 'frames.f32')) == 4 * (16 * hw + 48)


def test_presave_is_atomic(tmp_path, monkeypatch):
    """a failure while the new file is written leaves frames.npz as it was and no temporary file behind"""
    from depthinspace_amd.data import presave_sgm as P
    root, st, paths = _dataset(tmp_path, 1)
    path = os.path.join(paths[0], 'frames.npz')
    before = open(path, 'rb').read()
    monkeypatch.setattr(P, 'match_frames', _fake_matcher([]))
    real_savez = np.savez

    def failing_savez(file, **arrays):
        real_savez(file, **{k: v for k, v in arrays.items() if k == 'im'})       # a partial file ...
        raise OSError('disk full')                                               # ... and then the failure

    monkeypatch.setattr(P.np, 'savez', failing_savez)
    with pytest.raises(OSError):
        P.presave_sgm(root)
    monkeypatch.setattr(P.np, 'savez', real_savez)
    assert open(path, 'rb').read() == before and sorted(os.listdir(paths[0])) == ['flow.npz', 'frames.npz']
    replaced = []
    real_replace = os.replace
    monkeypatch.setattr(P.os, 'replace', lambda a, b: (replaced.append((a, b)), real_replace(a, b))[1])
    assert P.presave_sgm(root) == 1
    assert len(replaced) == 1 and replaced[0][1] == path and replaced[0][0] != path and os.path.dirname(replaced[0][0]) == paths[0]


def test_report_uses_the_projects_metrics(tmp_path, monkeypatch, capsys):
    from depthinspace_amd.data import presave_sgm as P
    root, st, paths = _dataset(tmp_path, 2)

    def match(im, pattern, *a, **k):   # the truth + 0.25 on the left half, + 3 on a quarter, invalid (0) on the rest
        for p in paths:
            with np.load(os.path.join(p, 'frames.npz')) as f:
                if np.array_equal(f['im'], im):
                    d = f['disp'].copy()
        d[..., :24] += 0.25
        d[..., 24:36] += 3
        d[..., 36:] = 0
        return d

    monkeypatch.setattr(P, 'match_frames', match)
    res = P.presave_sgm(root, report=True)
    assert 'valid 0.7500' in capsys.readouterr().out
    assert res['valid'] == pytest.approx(0.75)
    assert res['of1'] == pytest.approx(1.0 / 3.0) and res['of0.1'] == pytest.approx(1.0) and res['of5'] == 0.0
    assert res['dist2_median'] == pytest.approx(0.25, abs=1e-5) and res['dist2_max'] == pytest.approx(3.0, abs=1e-5)
