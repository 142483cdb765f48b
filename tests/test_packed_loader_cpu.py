"""CPU: packed track files (depthinspace_amd/data/packed.py) - the packer's round trip and incrementality, PackedTrackLoader
against TrackNpzDataset + collate through the numpy reference assembly (tests/packed_ref.py), batch order and determinism under
random reader timing, the staging ring's guard, the error paths, and the argument checks of dis_assemble_tracks (every refusal
returns before anything is launched: the library is reached as tests/test_abi.py reaches it)."""
import ctypes
import os
import random
import threading
import time

import numpy as np
import pytest
import torch

from depthinspace_amd.data import packed as P
from tests import packed_ref as R

SIZES = [(16, 20), (31, 33)]


def _lib():
    import __graft_entry__ as g
    from depthinspace_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    return lib


@pytest.fixture(scope='module')
def roots(tmp_path_factory):
    """packed roots of 6 tracks, read-only for the tests that share them: (h, w, sgm) -> (root, track directories)"""
    out = {}
    for h, w in SIZES:
        for sgm in (False, True):
            if sgm and (h, w) != SIZES[0]:
                continue
            root = str(tmp_path_factory.mktemp(f'packed_{h}x{w}_{int(sgm)}'))
            paths = R.make_root(root, h, w, 6, seed=50 + h, sgm=sgm)
            P.pack_dataset(root)
            out[(h, w, sgm)] = (root, paths)
    return out


def _run(fn, timeout=60):
    """fn() in a thread joined with a timeout: a loader that hangs fails the test instead of stalling it"""
    box = {}

    def body():
        try:
            box['ret'] = fn()
        except BaseException as e:
            box['exc'] = e
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(timeout)
    assert not t.is_alive(), 'the loader hangs'
    if 'exc' in box:
        raise box['exc']
    return box['ret']


def _loader(root, paths, h, w, **kw):
    args = dict(order=list(range(len(paths))), batch_size=2, track_length=4, train=True, imsize=(h, w), primary=True, pseudo=True,
                num_threads=2, seed=3, root=root)
    args.update(kw)
    return P.PackedTrackLoader(paths, **args)


# ---------------------------------------------------------------------------------------------------------------- the packer
@pytest.mark.parametrize('h,w,sgm', [(16, 20, False), (31, 33, False), (16, 20, True)])
def test_pack_round_trip_and_incremental(tmp_path, h, w, sgm):
    import json
    root = str(tmp_path)
    paths = R.make_root(root, h, w, 3, sgm=sgm)
    written = P.pack_dataset(root)
    assert len(written) == 4 * 3
    meta = json.load(open(os.path.join(root, 'packed.json')))
    assert meta == {'version': 1, 'imsize': [h, w],
                    'frames_fields': ['im', 'ambient', 'disp'] + (['sgm_disp'] if sgm else []) + ['R', 't']}
    for d in paths:
        fr, fl = np.load(os.path.join(d, 'frames.npz')), np.load(os.path.join(d, 'flow.npz'))
        names = ['im', 'ambient', 'disp'] + (['sgm_disp'] if sgm else []) + ['R', 't']
        assert open(os.path.join(d, 'frames.f32'), 'rb').read() == b''.join(fr[n].astype('<f4').tobytes() for n in names)
        assert open(os.path.join(d, 'flow.f32'), 'rb').read() == b''.join(fl['flow_' + p].astype('<f4').tobytes() for p in P.PAIRS)
        for stem in ('single_frame_disp', 'multi_frame_disp'):
            assert open(os.path.join(d, stem + '.f32'), 'rb').read() == np.load(os.path.join(d, stem + '.npz'))['disp'].tobytes()
    lay = P.record_layout(h, w, sgm, True, True)
    assert lay['size'] * 4 == sum(os.path.getsize(os.path.join(paths[0], s + '.f32')) for s in P.FILES)
    assert [f[0] for f in lay['files']] == list(P.FILES) and 'grad' not in lay
    # a second run rewrites nothing; a touched npz makes exactly that file stale
    before = {p: os.stat(p).st_mtime_ns for p in written}
    assert P.pack_dataset(root) == []
    assert {p: os.stat(p).st_mtime_ns for p in written} == before
    npz = os.path.join(paths[1], 'flow.npz')
    future = time.time() + 100
    os.utime(npz, (future, future))
    stale = [p for p in written if P.is_stale(p, p[:-4] + '.npz')]
    assert stale == [os.path.join(paths[1], 'flow.f32')]
    assert P.pack_dataset(root) == stale


def test_record_layout_alignment_and_stages():
    for h, w in ((16, 20), (512, 432)):
        hw = h * w
        for sgm in (False, True):
            lay = P.record_layout(h, w, sgm, True, True)
            for k in ('im', 'ambient', 'disp', 'flow', 'primary_disp', 'pseudo_gt') + (('sgm_disp',) if sgm else ()):
                assert lay[k] % 4 == 0 and lay['size'] % 4 == 0    # 16-byte aligned planes
            assert lay['R'] == (4 if sgm else 3) * 4 * hw and lay['t'] == lay['R'] + 36 and lay['flow'] == lay['t'] + 12
    sf = P.record_layout(16, 20, False, False, False)
    assert 'primary_disp' not in sf and 'pseudo_gt' not in sf and sf['size'] == (12 + 24) * 320 + 48
    ft = P.record_layout(16, 20, False, False, True)
    assert ft['pseudo_gt'] == sf['size'] and [f[0] for f in ft['files']] == ['frames', 'flow', 'multi_frame_disp']


# ------------------------------------------------------------------------------------------- loader == TrackNpzDataset + collate
@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('tl', [2, 3, 4])
@pytest.mark.parametrize('train', [True, False])
def test_loader_equals_npz_dataset(roots, h, w, tl, train):
    from depthinspace_amd.data.dataset import TrackNpzDataset, collate
    for sgm, primary, pseudo in ((False, True, True), (False, False, False), (True, True, False), (False, False, True)):
        if sgm and (h, w, True) not in roots:
            continue
        root, paths = roots[(h, w, sgm)]
        seed = 11 + tl
        order = [4, 0, 5, 2, 1]
        ds = TrackNpzDataset(root, paths, track_length=tl, train=train, load_flow_data=True, load_primary_data=primary,
                             load_pseudo_gt=pseudo, data_type='real' if sgm else 'synthetic')
        np.random.seed(seed)
        ref = [collate([ds[i] for i in order[k:k + 2]]) for k in range(0, len(order), 2)]
        ld = _loader(root, paths, h, w, order=order, track_length=tl, train=train, has_sgm=sgm, primary=primary, pseudo=pseudo,
                     seed=seed)
        assert len(ld) == 3

        def take():
            got = []
            for b in ld:
                assert b.perm.dtype == torch.int32 and tuple(b.perm.shape) == (b.bs, tl)
                got.append(R.assemble(b.raw.numpy().copy(), ld.record, b.perm.numpy().copy(), h, w, sgm, primary, pseudo))
            return got
        got = _run(take)
        assert len(got) == len(ref) and got[-1]['im0'].shape[1] == 1      # a smaller last batch without drop_last
        for g, r in zip(got, ref):
            r = R.collate_to_assembled(r)
            assert set(g) == set(r), set(g) ^ set(r)
            for k in r:
                assert g[k].dtype == np.float32 and np.array_equal(g[k], r[k]), k
        # drop_last, as Worker._loader asks for when training
        assert len(_loader(root, paths, h, w, order=order, track_length=tl, drop_last=True)) == 2


def test_loader_seed_follows_random_state(roots):
    root, paths = roots[(16, 20, False)]
    ld = _loader(root, paths, 16, 20, track_length=3, seed=77)
    perms = _run(lambda: [b.perm.numpy().copy() for b in ld])
    rng = np.random.RandomState(77)
    want = [np.stack([rng.permutation(4)[:3] for _ in range(2)]) for _ in range(3)]
    assert all(np.array_equal(a, b) for a, b in zip(perms, want))
    test = _loader(root, paths, 16, 20, track_length=3, train=False)
    assert all(np.array_equal(b.perm.numpy(), np.tile(np.arange(3), (2, 1))) for b in _run(lambda: list(test)))


# --------------------------------------------------------------------------------------------------- order, determinism, ring
def test_order_and_determinism_under_random_reader_timing(roots):
    root, paths = roots[(16, 20, False)]
    order = [3, 1, 4, 0, 2, 5, 1, 3]

    def run(delay_seed):
        rnd = random.Random(delay_seed)
        lock = threading.Lock()

        def slow_reader(path, buf):
            with lock:
                d = rnd.uniform(0.0, 0.004)
            time.sleep(d)
            P.read_exact(path, buf)
        ld = _loader(root, paths, 16, 20, order=order, num_threads=4, reader=slow_reader, seed=9)
        return _run(lambda: [(b.raw.numpy().tobytes(), b.perm.numpy().tobytes()) for b in ld])
    a, b = run(1), run(2)
    assert a == b and len(a) == 4
    # sampler order: record pos of batch k is track order[2k + pos]
    lay = P.record_layout(16, 20, False, True, True)
    for k, (raw, _) in enumerate(a):
        raw = np.frombuffer(raw, np.float32)
        for pos in range(2):
            want = np.load(os.path.join(paths[order[2 * k + pos]], 'frames.npz'))['im'].reshape(-1)
            assert np.array_equal(raw[pos * lay['size'] + lay['im']:][:want.size], want)


def test_ring_slot_is_refilled_only_behind_its_guard(roots):
    root, paths = roots[(16, 20, False)]
    log = []

    class Guard(object):
        def __init__(self):
            self.released = False

        def record(self, stream):
            log.append(('record', id(self)))

        def synchronize(self):
            self.released = True
            log.append(('sync', id(self)))
    ld = _loader(root, paths, 16, 20, order=list(range(6)) * 2, batch_size=2, num_threads=3, event_factory=Guard)
    bad = []

    def reader(path, buf):
        base = ctypes.addressof(ctypes.c_char.from_buffer(buf))
        for slot, hb in enumerate(ld._host_bytes):
            lo = ctypes.addressof(ctypes.c_char.from_buffer(hb))
            if lo <= base < lo + len(hb):
                g = ld._guard[slot]
                if g is not None and not g.released:
                    bad.append(slot)
        P.read_exact(path, buf)
    ld.reader = reader
    n = _run(lambda: sum(1 for _ in ld))
    assert n == 6 and not bad
    # every batch got a guard; all but the guards of the last `depth` batches were waited for before their slot was refilled
    recs = [g for kind, g in log if kind == 'record']
    syncs = [g for kind, g in log if kind == 'sync']
    assert len(recs) == 6 and syncs == recs[:6 - ld.depth]
    for g in syncs:
        assert log.index(('record', g)) < log.index(('sync', g))


# ------------------------------------------------------------------------------------------------------------------ error paths
def _broken_root(tmp_path, how):
    root = str(tmp_path)
    paths = R.make_root(root, 16, 20, 4)
    P.pack_dataset(root)
    victim = os.path.join(paths[2], 'flow.f32')
    if how == 'truncated':
        with open(victim, 'r+b') as fp:
            fp.truncate(os.path.getsize(victim) - 8)
    elif how == 'missing':
        os.remove(victim)
    elif how == 'stale':
        future = time.time() + 100
        os.utime(os.path.join(paths[2], 'flow.npz'), (future, future))
    return root, paths, victim


@pytest.mark.parametrize('how', ['truncated', 'missing', 'stale'])
def test_bad_files_raise_the_documented_error(tmp_path, how):
    root, paths, victim = _broken_root(tmp_path, how)
    ld = _loader(root, paths, 16, 20)
    it = iter(ld)
    assert _run(lambda: next(it)).bs == 2               # tracks 0, 1 are fine
    with pytest.raises(P.PackedDataError) as e:
        _run(lambda: next(it))                          # track 2 is not
    assert victim in str(e.value) and f'python -m depthinspace_amd.data.packed {root}' in str(e.value)
    _run(it.close)


def test_reader_exception_reaches_next(roots):
    root, paths = roots[(16, 20, False)]

    def reader(path, buf):
        if path.endswith(os.path.join(os.path.basename(paths[3]), 'frames.f32')):
            raise OSError('disk on fire')
        P.read_exact(path, buf)
    ld = _loader(root, paths, 16, 20, reader=reader, num_threads=4)
    it = iter(ld)
    _run(lambda: next(it))
    with pytest.raises(OSError, match='disk on fire'):
        _run(lambda: next(it))
    _run(it.close)


def test_loader_rejects_a_bad_frame_table(roots):
    root, paths = roots[(16, 20, False)]
    ld = _loader(root, paths, 16, 20)
    ld._draw = lambda n: np.array([[0, 1, 2, 2]] * n, np.int32)
    with pytest.raises(ValueError, match='frame order'):
        _run(lambda: next(iter(ld)))
    with pytest.raises(RuntimeError, match='HIP'):          # no host form of the assembly, no fallback
        ld2 = _loader(root, paths, 16, 20)
        _run(lambda: next(iter(ld2)).assemble())


def test_worker_selects_the_packed_loader_by_packed_json(tmp_path):
    """Worker._loader: a PackedTrackLoader iff <data_root>/packed.json exists, the DataLoader exactly as before otherwise"""
    import argparse
    from depthinspace_amd.model import multi_frame_worker
    root = str(tmp_path / 'data')
    R.make_root(root, 16, 20, 4, pseudo=False)
    args = argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic', architecture='multi_frame',
                              epochs=1, warmup_epochs=150, train_batch_size=2, max_disp=128)
    w = multi_frame_worker.Worker(args, data_root=root, num_workers=3, train_device='cpu', test_device='cpu')
    dset = w._make_dataset(sorted(os.path.join(root, d) for d in os.listdir(root) if d.startswith('0')), True, False, 0, 0)
    ld = w._loader(dset, 2, True, 0)
    assert isinstance(ld, torch.utils.data.DataLoader) and ld.num_workers == 3 and ld.drop_last
    P.pack_dataset(root)
    w.current_epoch = 2
    ld = w._loader(dset, 2, True, 2)
    assert isinstance(ld, P.PackedTrackLoader) and ld.num_threads == 3 and ld.drop_last and ld.primary and not ld.pseudo
    assert len(ld) == 2 and ld.device is None
    rng = np.random.RandomState((w.seed + 7919 * 2) % 2 ** 31)
    first = _run(lambda: next(iter(ld)))
    assert np.array_equal(first.perm.numpy(), np.stack([rng.permutation(4) for _ in range(2)]))
    w.num_workers = 64
    assert w._loader(dset, 2, False, 0).num_threads == 8 and not w._loader(dset, 2, False, 0).drop_last


# ----------------------------------------------------------------------------- dis_assemble_tracks: refusals without a GPU
def test_assemble_tracks_argument_checks():
    lib = _lib()
    f = lib.fn('dis_assemble_tracks')
    buf = ctypes.create_string_buffer(256)      # never dereferenced: every call below is refused on the host
    Pp = ctypes.cast(buf, ctypes.c_void_p).value
    BAD_SHAPE, UNSUPPORTED, NULL = -1, -2, -3
    h, w = 8, 12
    lay = P.record_layout(h, w, True, True, True)

    def structs(absent=(), out_absent=('sgm_disp', 'primary_disp', 'pseudo_gt'), **over):
        L, O = lib.TrackLayout(), lib.TrackOut()
        for n in lib.TRACK_FIELDS:
            setattr(L, n, -1 if n in absent else over.get(n, lay[n]))
            setattr(O, n, None if n in out_absent else Pp)
        return L, O

    def call(L, O, raw=Pp, perm=Pp, stride=lay['size'], bs=2, tl=4, hh=h, ww=w, layout=True, out=True):
        return f(raw, stride, perm, ctypes.addressof(L) if layout else None, ctypes.addressof(O) if out else None, bs, tl, hh, ww,
                 None)
    # 1. NULL: raw, perm, layout, out, a mandatory output - before any shape is looked at
    L, O = structs()
    assert call(L, O, raw=None) == NULL and call(L, O, perm=None) == NULL
    assert call(L, O, layout=False) == NULL and call(L, O, out=False) == NULL
    for n in ('im', 'ambient', 'disp', 'R', 't'):
        L, O = structs(out_absent=(n,))
        assert call(L, O) == NULL, n
        assert call(L, O, bs=0) == NULL and call(L, O, stride=1) == NULL, n
    # 2. bad shapes: extents, tl > 4, a field of the layout outside [0, record_stride)
    L, O = structs()
    for kw in (dict(bs=0), dict(bs=-1), dict(tl=0), dict(tl=5), dict(hh=0), dict(ww=-3)):
        assert call(L, O, **kw) == BAD_SHAPE, kw
    assert call(L, O, stride=lay['size'] - 1) == BAD_SHAPE       # the last field ends one float behind the record
    assert call(L, O, stride=0) == BAD_SHAPE and call(L, O, stride=-lay['size']) == BAD_SHAPE
    for n in lib.TRACK_FIELDS:
        for off in (-2, lay['size'], lay['size'] - 1, 1 << 40):
            L, O = structs(**{n: off})
            assert call(L, O) == BAD_SHAPE, (n, off)
        # ... also for a field no output asks for, and before the unsupported check
        L, O = structs(absent=('flow',), **{n: -7} if n != 'flow' else {'pseudo_gt': -7})
        assert call(L, O) == BAD_SHAPE, n
    # 3. an output whose field the layout lacks
    for n in lib.TRACK_FIELDS:
        L, O = structs(absent=(n,), out_absent=())
        assert call(L, O) == UNSUPPORTED, n
    # absent in both is fine for the optional fields - nothing left to refuse, so nothing is called here


def test_ops_wrapper_refuses_host_tensors():
    _lib()
    from depthinspace_amd import ops
    lay = P.record_layout(8, 12)
    with pytest.raises(RuntimeError, match='HIP'):
        ops.assemble_tracks(torch.zeros(lay['size']), torch.zeros((1, 2), dtype=torch.int32), 1, 2, 8, 12)
