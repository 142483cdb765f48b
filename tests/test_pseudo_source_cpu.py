"""CPU: the pseudo-GT source of a stage - TrackNpzDataset(pseudo_stem=...), record_layout with a stem, the packer on roots with and
without raycast files, and the loader's refusal of a stem that was not packed.  No device is used."""
import argparse
import json
import os

import numpy as np
import pytest

from depthinspace_amd.data import packed as P
from depthinspace_amd.data.dataset import TrackNpzDataset
from tests import packed_ref as R

H, W = 16, 20


def _raycast_file(d, stem='raycast_gt', holes=True):
    """a raycast_<disp>.npz as data/raycast.py writes it: disp (4,1,H,W) with zeros where no ray hit, normal, value"""
    with np.load(os.path.join(d, 'frames.npz')) as f:
        disp = (f['disp'] + 5.0).astype(np.float32)
    if holes:
        disp[:, :, 2:6, 3:9] = 0
    np.savez(os.path.join(d, stem + '.npz'), disp=disp, normal=np.zeros((4, 3, H, W), np.float32), value=np.ones((4, 1, H, W), np.float32))
    return disp


def _listing(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_dataset_reads_the_named_stem(tmp_path):
    root = str(tmp_path)
    paths = R.make_root(root, H, W, 2)
    want = [_raycast_file(d) for d in paths]
    ds = TrackNpzDataset(root, paths, track_length=3, train=False, load_pseudo_gt=True, pseudo_stem='raycast_gt')
    for i in range(2):
        got = ds[i]['pseudo_gt'].numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want[i][:3])     # test mode: frames 0, 1, 2 in order
    # the default argument still reads multi_frame_disp.npz
    dflt = TrackNpzDataset(root, paths, track_length=4, train=False, load_pseudo_gt=True)
    assert dflt.pseudo_stem == 'multi_frame_disp'
    with np.load(os.path.join(paths[0], 'multi_frame_disp.npz')) as f:
        assert np.array_equal(dflt[0]['pseudo_gt'].numpy(), f['disp'])
    assert 'pseudo_gt' not in TrackNpzDataset(root, paths, train=False, pseudo_stem='raycast_gt')[0]


def test_missing_file_names_path_and_command(tmp_path):
    root = str(tmp_path)
    paths = R.make_root(root, H, W, 1)
    ds = TrackNpzDataset(root, paths, train=False, load_pseudo_gt=True, pseudo_stem='raycast_sgm')
    with pytest.raises(FileNotFoundError) as e:
        ds[0]
    msg = str(e.value)
    assert os.path.join(paths[0], 'raycast_sgm.npz') in msg
    assert f'python -m depthinspace_amd.data.raycast {root} --disp sgm' in msg


def test_record_layout_with_a_stem():
    base = P.record_layout(H, W, False, True, True)
    assert P.record_layout(H, W, False, True, True, pseudo_stem='multi_frame_disp') == base
    assert [f[0] for f in base['files']] == ['frames', 'flow', 'single_frame_disp', 'multi_frame_disp']
    assert P.RAYCAST_FILES == ('raycast_gt', 'raycast_sgm', 'raycast_single_frame', 'raycast_multi_frame')
    for stem in P.RAYCAST_FILES:
        lay = P.record_layout(H, W, False, True, True, pseudo_stem=stem)
        assert [f[0] for f in lay['files']] == ['frames', 'flow', 'single_frame_disp', stem]
        assert [f[1:] for f in lay['files']] == [f[1:] for f in base['files']]
        assert {k: v for k, v in lay.items() if k != 'files'} == {k: v for k, v in base.items() if k != 'files'}
    # without pseudo-GT the stem is not read at all
    assert P.record_layout(H, W, True, True, False, pseudo_stem='raycast_gt') == P.record_layout(H, W, True, True, False)
    with pytest.raises(ValueError):
        P.record_layout(H, W, pseudo=True, pseudo_stem='frames')
    assert P.VERSION == 1 and P.FILES == ('frames', 'flow', 'single_frame_disp', 'multi_frame_disp')


def test_pack_with_and_without_raycast_files(tmp_path):
    plain, rc = str(tmp_path / 'plain'), str(tmp_path / 'rc')
    p0 = R.make_root(plain, H, W, 2, seed=7)
    p1 = R.make_root(rc, H, W, 2, seed=7)
    want = _raycast_file(p1[1])                                 # only the second track holds one
    w0, w1 = P.pack_dataset(plain), P.pack_dataset(rc)
    # without raycast files: the four files per track, in FILES order, and nothing else
    assert w0 == [os.path.join(d, s + '.f32') for d in p0 for s in P.FILES]
    assert _listing(plain) == sorted(['packed.json', 'settings.npz'] + [os.path.join(os.path.basename(d), s + e) for d in p0
                                                                         for s in P.FILES for e in ('.npz', '.f32')])
    assert json.load(open(os.path.join(plain, 'packed.json'))) == {'version': 1, 'imsize': [H, W],
                                                                    'frames_fields': ['im', 'ambient', 'disp', 'R', 't']}
    assert open(os.path.join(plain, 'packed.json'), 'rb').read() == open(os.path.join(rc, 'packed.json'), 'rb').read()
    for d0, d1 in zip(p0, p1):
        for s in P.FILES:                                       # records of the shared stems: byte-identical
            assert open(os.path.join(d0, s + '.f32'), 'rb').read() == open(os.path.join(d1, s + '.f32'), 'rb').read()
    # with one: its `disp` bytes, after the other files of that track
    extra = os.path.join(p1[1], 'raycast_gt.f32')
    assert w1 == [p.replace(plain, rc) for p in w0] + [extra]
    assert open(extra, 'rb').read() == want.astype('<f4').tobytes() and os.path.getsize(extra) == 4 * 4 * H * W
    assert not os.path.exists(os.path.join(p1[0], 'raycast_gt.f32'))
    assert P.pack_dataset(rc) == []                             # incremental like the rest
    _raycast_file(p1[0], 'raycast_single_frame')
    assert P.pack_dataset(rc) == [os.path.join(p1[0], 'raycast_single_frame.f32')]


def test_loader_reads_the_stem_and_never_another(tmp_path):
    root = str(tmp_path)
    paths = R.make_root(root, H, W, 2)
    want = [_raycast_file(d) for d in paths]
    P.pack_dataset(root)
    kw = dict(order=[0, 1], batch_size=2, track_length=4, train=False, imsize=(H, W), primary=False, pseudo=True, num_threads=1, root=root)
    ld = P.PackedTrackLoader(paths, pseudo_stem='raycast_gt', **kw)
    assert ld.record == P.PackedTrackLoader(paths, **kw).record
    (b,) = list(ld)
    raw = b.raw.numpy().reshape(2, ld.record)
    off = ld.layout['pseudo_gt']
    for i in range(2):
        assert np.array_equal(raw[i, off:off + 4 * H * W].reshape(4, 1, H, W), want[i])
    # a stem that was never packed: PackedDataError with the pack command, although multi_frame_disp.f32 lies next to it
    _raycast_file(paths[0], 'raycast_sgm')
    with pytest.raises(P.PackedDataError) as e:
        list(P.PackedTrackLoader(paths, pseudo_stem='raycast_sgm', **kw))
    assert 'raycast_sgm.f32' in str(e.value) and P.pack_command(root) in str(e.value)
    # ... and one that no track holds at all: the raycast command is named too
    with pytest.raises(P.PackedDataError) as e:
        list(P.PackedTrackLoader(paths, pseudo_stem='raycast_multi_frame', **kw))
    msg = str(e.value)
    assert 'raycast_multi_frame.f32' in msg and P.pack_command(root) in msg and '--disp multi_frame' in msg


def test_loader_for_takes_the_stem_from_the_dataset(tmp_path):
    root = str(tmp_path)
    paths = R.make_root(root, H, W, 2)
    for d in paths:
        _raycast_file(d)
    P.pack_dataset(root)
    ds = TrackNpzDataset(root, paths, train=False, load_flow_data=True, load_pseudo_gt=True, pseudo_stem='raycast_gt')
    ld = P.loader_for(ds, [0, 1], 1, False, 1, 0, None, root)
    assert ld.pseudo_stem == 'raycast_gt' and ld.layout['files'][-1][0] == 'raycast_gt'
    dflt = TrackNpzDataset(root, paths, train=False, load_flow_data=True, load_pseudo_gt=True)
    assert P.loader_for(dflt, [0, 1], 1, False, 1, 0, None, root).layout['files'][-1][0] == 'multi_frame_disp'


def test_flags_and_stems():
    from depthinspace_amd.co.args import parse_args, pseudo_gt_stem, PSEUDO_GT_SOURCES
    a = parse_args([])
    assert a.pseudo_gt_source == 'multi_frame' and a.pseudo_gt_erode == 0
    a = parse_args(['--pseudo_gt_source', 'raycast_sgm', '--pseudo_gt_erode', '2'])
    assert a.pseudo_gt_source == 'raycast_sgm' and a.pseudo_gt_erode == 2
    for bad in (['--pseudo_gt_source', 'raycast'], ['--pseudo_gt_erode', '4'], ['--pseudo_gt_erode', '-1']):
        with pytest.raises(SystemExit):
            parse_args(bad)
    assert [pseudo_gt_stem(s) for s in PSEUDO_GT_SOURCES] == ['multi_frame_disp'] + list(P.RAYCAST_FILES)
    with pytest.raises(ValueError):
        pseudo_gt_stem('sgm')


def test_worker_reads_the_fields_with_defaults():
    """a Namespace without the new fields (every existing test builds one) means the reference's pseudo-GT"""
    from depthinspace_amd import synth
    from depthinspace_amd.model import single_frame_worker
    ns = dict(use_pseudo_gt=True, lcn_radius=5, track_length=4, data_type='synthetic', architecture='single_frame', epochs=1,
              warmup_epochs=150, train_batch_size=1, max_disp=128)
    st = synth.make_settings(64, 64)
    w = single_frame_worker.Worker(argparse.Namespace(**ns), settings=st)
    assert (w.pseudo_gt_source, w.pseudo_gt_erode, w.pseudo_gt_stem) == ('multi_frame', 0, 'multi_frame_disp')
    w = single_frame_worker.Worker(argparse.Namespace(pseudo_gt_source='raycast_gt', pseudo_gt_erode=1, **ns), settings=st)
    assert (w.pseudo_gt_source, w.pseudo_gt_erode, w.pseudo_gt_stem) == ('raycast_gt', 1, 'raycast_gt')
    with pytest.raises(ValueError):
        single_frame_worker.Worker(argparse.Namespace(pseudo_gt_source='raycast', **ns), settings=st)
    with pytest.raises(ValueError):
        single_frame_worker.Worker(argparse.Namespace(pseudo_gt_erode=4, **ns), settings=st)
