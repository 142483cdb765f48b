"""Packed track files and their loader: on-disk training at the step's own rate.

The .npz schema of dataset.py stays the exchange format.  Next to each .npz of a track directory the packer writes the same
arrays, bit for bit, as one raw little-endian fp32 file:
    frames.f32                im (4,H,W) | ambient (4,H,W) | disp (4,H,W) | [sgm_disp (4,H,W)] | R (4,3,3) | t (4,3)
    flow.f32                  flow_ij (2,H,W) in the order 01 02 03 10 12 13 20 21 23 30 31 32
    single_frame_disp.f32     disp (4,H,W)          multi_frame_disp.f32      disp (4,H,W)
    raycast_<disp>.f32        disp (4,H,W) of raycast_<disp>.npz, where a track holds one (a pseudo-GT source; normal and value are not packed)
(`grad` is not stored: nothing reads it.  R and t come last, so the image planes stay 16-byte aligned when H*W % 4 == 0.)
<root>/packed.json holds the version, imsize and the field list of frames.f32; its presence selects this path in Worker._loader.

A *record* is what one stage reads of one track: frames | flow | single_frame_disp (if the stage loads it) | multi_frame_disp, or the
raycast file the stage names instead (if pseudo-GT).  record_layout() is the one place that knows the offsets: the packer, the loader and ops.assemble_tracks use it.

PackedTrackLoader reads the records with a thread pool (file reads release the GIL: no worker processes, no pickling) straight into
a pinned staging ring, uploads each batch with ONE copy on its own stream while the previous step runs, and hands out PackedBatch
objects; the frame permutation, the transposes and the flow stacking happen on the device in one launch (dis_assemble_tracks).

    python -m depthinspace_amd.data.packed ROOT        # (re)pack what is missing or older than its .npz
"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .trackfiles import SOURCES

VERSION = 1
PAIRS = tuple(f'{i}{j}' for i in range(4) for j in range(4) if i != j)   # file order of the flows: pair(p, q) = 3p + q - (q > p)
FILES = ('frames', 'flow', 'single_frame_disp', 'multi_frame_disp')
# pseudo-GT of another stem (data/raycast.py writes them; only `disp` is packed): packed where a track holds the .npz
RAYCAST_FILES = tuple(f'raycast_{s}' for s in SOURCES)


def pack_command(root):
    return f'python -m depthinspace_amd.data.packed {root}'


class PackedDataError(RuntimeError):
    """a packed file is missing, truncated or older than its .npz; the message names the pack command"""


class AssembledBatch(dict):
    """a batch already on the device and already in the (tl, bs, ...) layout of Worker.data (ops.assemble_tracks): copy_data takes
    its tensors as they are"""


def record_layout(h, w, has_sgm=False, primary=False, pseudo=False, pseudo_stem='multi_frame_disp'):
    """float offsets of every field of a record (keys: the field names of DisTrackLayout), plus
    'size' (floats per record) and 'files': ((file stem, float offset, floats), ...) in record order.  pseudo_stem: the file the
    pseudo_gt plane is read from (multi_frame_disp, or one of RAYCAST_FILES); sizes and offsets do not depend on it."""
    if pseudo_stem != 'multi_frame_disp' and pseudo_stem not in RAYCAST_FILES:
        raise ValueError(f'pseudo_stem is multi_frame_disp or one of {RAYCAST_FILES}, not {pseudo_stem!r}')
    hw = int(h) * int(w)
    lay, off = {}, 0
    for name in ('im', 'ambient', 'disp') + (('sgm_disp',) if has_sgm else ()):
        lay[name] = off
        off += 4 * hw
    lay['R'] = off
    lay['t'] = off + 36
    files = [('frames', 0, off + 48)]
    off += 48
    lay['flow'] = off
    files.append(('flow', off, 24 * hw))
    off += 24 * hw
    for on, name, stem in ((primary, 'primary_disp', 'single_frame_disp'), (pseudo, 'pseudo_gt', pseudo_stem)):
        if on:
            lay[name] = off
            files.append((stem, off, 4 * hw))
            off += 4 * hw
    lay['size'] = off
    lay['files'] = tuple(files)
    return lay


# ---------------------------------------------------------------------------------------------------------------------- packer
def _f32(a, shape):
    a = np.ascontiguousarray(a, dtype='<f4')
    if a.size != int(np.prod(shape)):
        raise ValueError(f'array of shape {a.shape} where {shape} is expected')
    return a.reshape(-1)


def _file_arrays(stem, f, h, w, has_sgm):
    """the arrays of one .npz (an open NpzFile) in the order of its .f32"""
    if stem == 'frames':
        names = ['im', 'ambient', 'disp'] + (['sgm_disp'] if has_sgm else [])
        return [_f32(f[n], (4, h, w)) for n in names] + [_f32(f['R'], (4, 3, 3)), _f32(f['t'], (4, 3))]
    if stem == 'flow':
        return [_f32(f[f'flow_{p}'], (2, h, w)) for p in PAIRS]
    return [_f32(f['disp'], (4, h, w))]


def is_stale(f32_path, npz_path):
    """missing, or older than its .npz"""
    try:
        return os.stat(f32_path).st_mtime_ns < os.stat(npz_path).st_mtime_ns
    except FileNotFoundError:
        return True


def track_dirs(root):
    return sorted(os.path.join(root, d) for d in os.listdir(root)
                  if os.path.isfile(os.path.join(root, d, 'frames.npz')))


def read_meta(root):
    with open(os.path.join(root, 'packed.json')) as fp:
        meta = json.load(fp)
    if meta.get('version') != VERSION:
        raise PackedDataError(f'{root}/packed.json has version {meta.get("version")}, this code reads {VERSION}: run '
                              f'`{pack_command(root)}`')
    return meta


def pack_dataset(root):
    """Writes <track>/<stem>.f32 for every <track>/<stem>.npz of `root` that has none or a newer .npz (incremental), then
    <root>/packed.json.  Returns the list of files written."""
    root = str(root)
    dirs = track_dirs(root)
    if not dirs:
        raise ValueError(f'{root}: no track directories (…/frames.npz)')
    with np.load(os.path.join(dirs[0], 'frames.npz')) as f:
        has_sgm = 'sgm_disp' in f.files
        h, w = (int(v) for v in f['im'].shape[-2:])
    written = []
    for d in dirs:
        for stem in FILES + RAYCAST_FILES:
            src, dst = os.path.join(d, stem + '.npz'), os.path.join(d, stem + '.f32')
            if not os.path.exists(src) or not is_stale(dst, src):
                continue
            with np.load(src) as f:
                if stem == 'frames' and ('sgm_disp' in f.files) != has_sgm:
                    raise ValueError(f'{src}: sgm_disp is {"missing" if has_sgm else "present"}, unlike {dirs[0]}')
                arrays = _file_arrays(stem, f, h, w, has_sgm)
            tmp = dst + '.tmp'
            with open(tmp, 'wb') as fp:
                for a in arrays:
                    fp.write(memoryview(a).cast('B'))
            os.replace(tmp, dst)
            written.append(dst)
    fields = ['im', 'ambient', 'disp'] + (['sgm_disp'] if has_sgm else []) + ['R', 't']
    meta = {'version': VERSION, 'imsize': [h, w], 'frames_fields': fields}
    path = os.path.join(root, 'packed.json')
    old = None
    if os.path.exists(path):
        with open(path) as fp:
            old = json.load(fp)
    if old != meta:
        with open(path + '.tmp', 'w') as fp:
            json.dump(meta, fp, indent=1)
        os.replace(path + '.tmp', path)
    return written


# ---------------------------------------------------------------------------------------------------------------------- loader
def read_exact(path, buf):
    """fill the writable byte buffer `buf` from `path` with readinto (releases the GIL); the file must hold exactly len(buf) bytes"""
    with open(path, 'rb', buffering=0) as fp:
        size = os.fstat(fp.fileno()).st_size
        if size != len(buf):
            raise PackedDataError(f'{path}: {size} bytes where {len(buf)} are expected (truncated or of another stage / image '
                                  f'size)')
        got = 0
        while got < len(buf):
            n = fp.readinto(buf[got:])
            if not n:
                raise PackedDataError(f'{path}: short read, {got} of {len(buf)} bytes')
            got += n


class PackedBatch(object):
    """One batch of records as the loader hands it out: `raw` (bs * record floats) and `perm` (bs, tl) int32 - on the device, with
    their upload possibly still in flight on the loader's copy stream (`ready`), or, from a loader without a device, host views of
    the staging slot (valid until the next batch is asked for)."""

    def __init__(self, loader, index, slot, raw, perm, bs, ready=None):
        self.loader, self.index, self.slot, self.raw, self.perm, self.bs, self.ready = loader, index, slot, raw, perm, bs, ready
        self.tl = loader.track_length
        self.h, self.w = loader.imsize
        self.released = ready is None

    def signature(self):
        ld = self.loader
        return ('packed', self.bs, self.tl, self.h, self.w, ld.has_sgm, ld.primary, ld.pseudo, ld.want_sgm)

    def assemble(self, out=None, release=True):
        """the batch in its final layout (ops.assemble_tracks, on the current stream, which first waits for the upload); with
        release=True the device slot is handed back to the loader behind this launch"""
        from .. import ops
        ld = self.loader
        if self.ready is None:
            raise RuntimeError('PackedBatch.assemble: the loader has no device; batch assembly is a HIP kernel, there is no host '
                               'form')
        stream = torch.cuda.current_stream(self.raw.device)
        stream.wait_event(self.ready)
        res = ops.assemble_tracks(self.raw, self.perm, self.bs, self.tl, self.h, self.w, has_sgm=ld.has_sgm, primary=ld.primary,
                                  pseudo=ld.pseudo, want_sgm=ld.want_sgm, out=out)
        if release:
            self.release(stream)
        return res

    def release(self, stream=None):
        """everything `stream` (default: the current one) has been given so far is the last reader of this batch's device slot"""
        if self.ready is not None:
            self.loader._slot_free(self.slot, stream if stream is not None else torch.cuda.current_stream(self.raw.device))
            self.released = True


class PackedTrackLoader(object):
    """Iterates like the DataLoader(TrackNpzDataset) it replaces, over `order` (a ShardSampler's indices into `sample_paths`).

    num_threads reader threads fill a ring of `depth` >= 2 host slots (pinned when a CUDA device is present); the threads make no
    HIP calls.  Batches come out in `order` whatever the thread timing.  train: the frame order of every sample is
    rng.permutation(4)[:tl], drawn in batch order from RandomState(seed) - what TrackNpzDataset draws from numpy's global generator
    in a single loader process - else arange(tl); it is only RECORDED here, as an int32 (bs, tl) table, and applied on the device.
    device: the loader owns one copy stream and a two-slot device ring; next() waits for the batch's reads, enqueues one copy of
    the records and one of the table, records an event and returns.  Events, never a device-wide synchronisation, hold that
      * a host slot is refilled only after its upload has completed (the refill is issued by the NEXT call of next(), when it has),
      * a device slot is overwritten only after the assembly that read it (PackedBatch.release; a batch never released is
        covered by everything the consumer's current stream holds when the slot comes round again),
      * the consumer's stream waits for the upload before it reads (PackedBatch.assemble).
    event_factory: what makes the guard of a host slot (tests); reader: read_exact (tests)."""

    def __init__(self, sample_paths, order, batch_size, track_length, train, imsize, has_sgm=False, primary=False, pseudo=False,
                 want_sgm=None, drop_last=False, num_threads=4, seed=0, device=None, depth=2, reader=None, event_factory=None,
                 root=None, pseudo_stem='multi_frame_disp'):
        assert 1 <= track_length <= 4 and batch_size >= 1 and depth >= 2
        self.sample_paths = list(sample_paths)
        self.order = [int(i) for i in order]
        self.batch_size, self.track_length, self.train = int(batch_size), int(track_length), bool(train)
        self.imsize = (int(imsize[0]), int(imsize[1]))
        self.has_sgm, self.primary, self.pseudo = bool(has_sgm), bool(primary), bool(pseudo)
        self.want_sgm = self.has_sgm if want_sgm is None else bool(want_sgm)
        if self.want_sgm and not self.has_sgm:
            raise PackedDataError('the stage reads sgm_disp, which the packed frames do not hold')
        self.drop_last = bool(drop_last)
        self.num_threads = max(1, int(num_threads))
        self.rng = np.random.RandomState(int(seed) % (2 ** 31))
        self.depth = int(depth)
        self.reader = reader or read_exact
        self.root = root if root is not None else (os.path.dirname(self.sample_paths[0]) if self.sample_paths else '.')
        self.pseudo_stem = pseudo_stem
        self.layout = record_layout(self.imsize[0], self.imsize[1], self.has_sgm, self.primary, self.pseudo, pseudo_stem)
        self.record = self.layout['size']
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type != 'cuda':
            raise ValueError('PackedTrackLoader: device must be a CUDA(HIP) device or None')
        pin = torch.cuda.is_available()
        n = self.batch_size * self.record
        self.host = [torch.empty(n, dtype=torch.float32, pin_memory=pin) for _ in range(self.depth)]
        self.host_perm = [torch.zeros((self.batch_size, self.track_length), dtype=torch.int32, pin_memory=pin)
                          for _ in range(self.depth)]
        self._host_bytes = [memoryview(t.numpy()).cast('B') for t in self.host]
        self._guard = [None] * self.depth      # per host slot: the event behind its upload (None: free)
        self.event_factory = event_factory
        if self.device is not None:
            self.copy_stream = torch.cuda.Stream(device=self.device)
            self.dev = [torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(2)]
            self.dev_perm = [torch.zeros((self.batch_size, self.track_length), dtype=torch.int32, device=self.device)
                             for _ in range(2)]
            self._dev_free = [None, None]      # per device slot: the event behind its last reader (None: never used / unknown)
            self._dev_out = [None, None]       # per device slot: the batch that is out
            if self.event_factory is None:
                self.event_factory = torch.cuda.Event

    def __len__(self):
        n = len(self.order)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    # ---- reader threads: host code only
    def _read_track(self, path, slot, pos):
        base = (pos * self.record) * 4
        for stem, off, count in self.layout['files']:
            f32, npz = os.path.join(path, stem + '.f32'), os.path.join(path, stem + '.npz')
            try:
                if os.path.exists(npz) and is_stale(f32, npz):
                    raise PackedDataError(f'{f32} is missing or older than {stem}.npz')
                self.reader(f32, self._host_bytes[slot][base + off * 4: base + (off + count) * 4])
            except FileNotFoundError as e:
                first = ''
                if stem in RAYCAST_FILES and not os.path.exists(npz):   # (no .npz to pack either: name what writes it)
                    first = f'`python -m depthinspace_amd.data.raycast {self.root} --disp {stem[len("raycast_"):]}`, then '
                raise PackedDataError(f'{f32} is missing: run {first}`{pack_command(self.root)}`') from e
            except PackedDataError as e:
                if 'run `' in str(e):
                    raise
                raise PackedDataError(f'{e}: run `{pack_command(self.root)}`') from e

    def _slot_free(self, slot, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self._dev_free[slot] = ev
        self._dev_out[slot] = None

    def _draw(self, n):
        tl = self.track_length
        if self.train:
            return np.stack([self.rng.permutation(4)[:tl] for _ in range(n)]).astype(np.int32)
        return np.tile(np.arange(tl, dtype=np.int32), (n, 1))

    def __iter__(self):
        nb, bs = len(self), self.batch_size
        batches = [self.order[k * bs:(k + 1) * bs] for k in range(nb)]
        perms = [self._draw(len(b)) for b in batches]     # in batch order, before any thread runs
        pool = ThreadPoolExecutor(max_workers=self.num_threads, thread_name_prefix='packed-reader')
        futs = {}

        def submit(k):
            slot = k % self.depth
            g = self._guard[slot]
            if g is not None:          # the upload that read this slot: completed before a thread writes into it
                g.synchronize()
                self._guard[slot] = None
            futs[k] = [pool.submit(self._read_track, self.sample_paths[i], slot, pos) for pos, i in enumerate(batches[k])]

        try:
            for k in range(min(self.depth, nb)):
                submit(k)
            for k in range(nb):
                if k >= 1 and k - 1 + self.depth < nb and (k - 1 + self.depth) not in futs:
                    submit(k - 1 + self.depth)   # the slot of batch k - 1: its consumer has moved on, its upload is a step old
                err = None
                for f in futs.pop(k):
                    try:
                        f.result()
                    except BaseException as e:   # (wait for every read of the batch: no thread may still write into the slot)
                        err = err or e
                if err is not None:
                    raise err
                yield self._emit(k, k % self.depth, len(batches[k]), perms[k])
        finally:
            for fl in futs.values():
                for f in fl:
                    f.cancel()
            pool.shutdown(wait=True)

    def _emit(self, k, slot, n, perm):
        tl = self.track_length
        if perm.shape != (n, tl) or perm.min() < 0 or perm.max() > 3 or any(len(set(r)) != tl for r in perm.tolist()):
            raise ValueError(f'PackedTrackLoader: batch {k}: not a frame order table: {perm.tolist()}')
        self.host_perm[slot][:n] = torch.from_numpy(perm)
        if self.device is None:
            if self.event_factory is not None:   # (tests: a guard object stands where the upload's event would)
                self._guard[slot] = self.event_factory()
                self._guard[slot].record(None)
            return PackedBatch(self, k, slot, self.host[slot][:n * self.record], self.host_perm[slot][:n], n)
        ds = k % 2
        if self._dev_out[ds] is not None:      # handed out two batches ago and never released: whatever the consumer has enqueued
            self._dev_out[ds].release()
        with torch.cuda.stream(self.copy_stream):
            if self._dev_free[ds] is not None:
                self.copy_stream.wait_event(self._dev_free[ds])
            raw = self.dev[ds][:n * self.record]
            dperm = self.dev_perm[ds][:n]
            raw.copy_(self.host[slot][:n * self.record], non_blocking=True)
            dperm.copy_(self.host_perm[slot][:n], non_blocking=True)
            ev = self.event_factory()
            ev.record(self.copy_stream)
        self._guard[slot] = ev
        batch = PackedBatch(self, k, ds, raw, dperm, n, ready=ev)
        self._dev_out[ds] = batch
        return batch


def loader_for(dset, order, batch_size, train, num_threads, seed, device, root):
    """the PackedTrackLoader that stands in for DataLoader(dset: a TrackNpzDataset) on a packed root"""
    meta = read_meta(root)
    imsize = tuple(int(v) for v in meta['imsize'])
    if imsize != tuple(int(v) for v in dset.settings.imsize):
        raise PackedDataError(f'{root}/packed.json is for images of {imsize}, settings.npz says {tuple(dset.settings.imsize)}: run '
                              f'`{pack_command(root)}`')
    return PackedTrackLoader(dset.sample_paths, order, batch_size, dset.track_length, train, imsize,
                             has_sgm='sgm_disp' in meta['frames_fields'], primary=dset.load_primary_data,
                             pseudo=dset.load_pseudo_gt, want_sgm=dset.data_type == 'real', drop_last=train,
                             num_threads=num_threads, seed=seed, device=device, root=root,
                             pseudo_stem=getattr(dset, 'pseudo_stem', 'multi_frame_disp'))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python -m depthinspace_amd.data.packed ROOT')
    files = pack_dataset(sys.argv[1])
    print(f'{len(files)} files written under {sys.argv[1]}')
