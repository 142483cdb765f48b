"""CPU: data/trackfiles.py - the loaders and the atomic npz writer that the track tools share - on 2-frame 4 x 6 arrays."""
import os

import numpy as np
import pytest

from depthinspace_amd.data import trackfiles as TF

TL, H, W = 2, 4, 6


def _arrays():
    rng = np.random.RandomState(3)
    disp = rng.uniform(1, 9, (TL, 1, H, W)).astype(np.float32)
    return {'im': rng.uniform(0, 1, (TL, 1, H, W)).astype(np.float32), 'ambient': rng.uniform(0, 1, (TL, 1, H, W)).astype(np.float32),
            'disp': disp, 'sgm_disp': disp + 1, 'R': np.stack([np.eye(3, dtype=np.float32)] * TL), 't': rng.randn(TL, 3).astype(np.float32),
            'ids': np.arange(5, dtype=np.int64)}


@pytest.fixture
def track(tmp_path):
    d, a = str(tmp_path), _arrays()
    np.savez(os.path.join(d, 'frames.npz'), **a)
    for k, source in enumerate(('single_frame', 'multi_frame')):
        np.savez(os.path.join(d, f'{source}_disp.npz'), disp=a['disp'] + 2 + k)
    return d, a


def _bytes_of(path):
    with np.load(path) as f:
        return {k: (f[k].dtype, f[k].shape, f[k].tobytes()) for k in f.files}


def test_rewrite_adds_and_replaces_and_leaves_the_rest_byte_for_byte(track):
    d, a = track
    path = os.path.join(d, 'frames.npz')
    before = _bytes_of(path)
    new_t, flag = np.ones((TL, 3), np.float64), np.array([7], dtype=np.uint8)
    TF.rewrite_npz(path, {'t': new_t, 'flag': flag})
    after = _bytes_of(path)
    assert set(after) == set(before) | {'flag'}
    for k in before:
        if k != 't':
            assert after[k] == before[k], k
    assert after['t'] == (new_t.dtype, new_t.shape, new_t.tobytes()) and after['flag'] == (flag.dtype, flag.shape, flag.tobytes())
    assert sorted(os.listdir(d)) == ['frames.npz', 'multi_frame_disp.npz', 'single_frame_disp.npz']


def test_write_replaces_the_whole_file(tmp_path):
    path = os.path.join(str(tmp_path), 'flow.npz')
    TF.write_npz(path, {'a': np.zeros(3, np.float32), 'b': np.ones(2, np.int32)})
    TF.write_npz(path, {'c': np.full((2, 2), 5, np.float32)})
    got = _bytes_of(path)
    assert list(got) == ['c'] and got['c'] == (np.dtype(np.float32), (2, 2), np.full((2, 2), 5, np.float32).tobytes())
    assert os.listdir(str(tmp_path)) == ['flow.npz']


class _Unstorable:
    def __reduce__(self):
        raise TypeError('cannot be stored')


def test_a_failed_write_leaves_the_file_and_no_temporary(track):
    d, _ = track
    path = os.path.join(d, 'frames.npz')
    with open(path, 'rb') as fp:
        before = fp.read()
    with pytest.raises(Exception):
        TF.rewrite_npz(path, {'bad': np.array([_Unstorable()], dtype=object)})
    with pytest.raises(Exception):
        TF.write_npz(path, {'bad': np.array([_Unstorable()], dtype=object)})
    with pytest.raises(OSError):
        TF.write_npz(os.path.join(d, 'no_such_directory', 'x.npz'), {'a': np.zeros(2)})
    with open(path, 'rb') as fp:
        assert fp.read() == before
    assert not [n for n in os.listdir(d) if n.endswith('.tmp.npz')]


def test_load_track_takes_its_disparities_from_load_disp(track):
    d, a = track
    expected = {'gt': a['disp'], 'sgm': a['sgm_disp'], 'single_frame': a['disp'] + 2, 'multi_frame': a['disp'] + 3}
    assert set(expected) == set(TF.SOURCES)
    for source in TF.SOURCES:
        disp = TF.load_disp(d, source)
        assert disp.dtype == np.float32 and disp.shape == (TL, H, W) and disp.tobytes() == expected[source][:, 0].tobytes()
        got = TF.load_track(d, source)
        assert got[0].dtype == disp.dtype and got[0].shape == disp.shape and got[0].tobytes() == disp.tobytes()
        assert np.array_equal(got[1], a['R']) and np.array_equal(got[2], a['t'])
        assert np.array_equal(got[3], a['ambient'][:, 0]) and np.array_equal(got[4], a['disp'][:, 0])


def test_the_names_stay_where_the_tools_import_them():
    from depthinspace_amd.data import fuse, presave_pose
    assert fuse.SOURCES is TF.SOURCES and fuse.load_track is TF.load_track and presave_pose.load_disp is TF.load_disp
    assert callable(presave_pose.load_flow) and callable(presave_pose.stored_poses)


def test_refusals(track):
    d, a = track
    for load in (TF.load_disp, TF.load_track):
        with pytest.raises(ValueError):
            load(d, 'other')
    os.remove(os.path.join(d, 'single_frame_disp.npz'))
    for load in (TF.load_disp, TF.load_track):
        with pytest.raises(ValueError):
            load(d, 'single_frame')
    np.savez(os.path.join(d, 'frames.npz'), **{k: v for k, v in a.items() if k not in ('R', 'sgm_disp', 'disp')})
    with pytest.raises(KeyError):
        TF.load_track(d, 'multi_frame')          # no poses
    assert TF.load_disp(d, 'multi_frame').shape == (TL, H, W)
    for source in ('gt', 'sgm'):
        with pytest.raises(ValueError):
            TF.load_disp(d, source)              # frames.npz without the array
    np.savez(os.path.join(d, 'frames.npz'), **{k: v for k, v in a.items() if k != 'disp'})
    assert TF.load_track(d, 'sgm')[4] is None    # no ground truth stored
    with pytest.raises(ValueError):
        TF.load_track(d, 'gt')


def test_report_text_is_the_line_the_tools_print():
    res = {'valid': 0.5, 'points': 12, 'resid': float('nan'), 'name': 'x'}
    assert TF.report_text(res, '.6f') == 'valid 0.500000  points 12  resid nan  name x'
    assert TF.report_text({'ok': 3, 'share': 0.25}, '.6g') == 'ok 3  share 0.25'
    assert TF.report_text({'epe': 1.0}, '.4f') == 'epe 1.0000'
