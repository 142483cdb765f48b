"""Loader rates for on-disk training (profiles/r12_packed_loader.md): the .npz DataLoader against the packed-file loader.

    python scripts/loader_rate.py host [--tracks 64]        # CPU only: host side of both loaders, tracks/s
    python scripts/loader_rate.py e2e  [--steps 44]         # MI355X: DIS-MF bs=4, captured step, three legs, frames/s

host: 512x432, 8 generated tracks cycled, page cache warm (every file is read once before the timed passes).  The parent's
  DataLoader(TrackNpzDataset, bs=4, num_workers=4, collate) - worker start-up excluded: the clock starts at the first batch - against
  PackedTrackLoader without a device at 1, 2 and 4 threads.  Condition printed: packed at 4 threads >= 4 x the DataLoader.
e2e: 16 generated tracks cycled, DIS-MF bs=4 with the graph on, legs alternated `--rounds` times:
  (a) the .npz root through the DataLoader of Worker._loader (4 worker processes, pinned, same sampler and collate; the workers are
  SPAWNED: forked from a process that has initialised HIP they died of a segmentation fault on the MI355X host), (b) the packed copy
  of it through Worker._loader, (c) GraphedStep replays on a resident batch
  (bench.py's loop).  Every leg runs 4 untimed steps, then `--steps` timed ones, device synchronised at both ends.
One JSON line per result."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from depthinspace_amd import synth                                   # noqa: E402
from depthinspace_amd.data import dataset as D, packed as P          # noqa: E402

H, W, BS, TL = 512, 432, 4, 4


def make_roots(base, n):
    npz, packed = os.path.join(base, 'npz'), os.path.join(base, 'packed')
    paths = D.write_synthetic_dataset(npz, synth.make_settings(H, W), n, seed=70)
    for d in paths:   # DIS-MF reads the DIS-SF disparities: any stored disparity will do
        with np.load(os.path.join(d, 'frames.npz')) as f:
            np.savez(os.path.join(d, 'single_frame_disp.npz'), disp=f['disp'])
    shutil.copytree(npz, packed)
    P.pack_dataset(packed)
    for root in (npz, packed):   # page cache warm
        for dp, _, files in os.walk(root):
            for fn in files:
                with open(os.path.join(dp, fn), 'rb') as fp:
                    while fp.read(1 << 24):
                        pass
    return npz, packed


def _tracks(root):
    return sorted(os.path.join(root, d) for d in os.listdir(root) if d.startswith('0'))


def _seed_worker(worker_id):
    np.random.seed(1234 + worker_id)


def _timed(it, n_skip=0):
    """iterate; the clock starts after `n_skip` + 1 batches (start-up excluded) -> (batches timed, seconds)"""
    n, t0 = 0, None
    for k, _ in enumerate(it):
        if k == n_skip:
            t0 = time.perf_counter()
        elif k > n_skip:
            n += 1
    return n, time.perf_counter() - t0


def host(args):
    base = tempfile.mkdtemp(prefix='loader_rate_')
    try:
        npz, packed = make_roots(base, 8)
        order = [i % 8 for i in range(args.tracks + BS)]       # (+ the untimed first batch)
        cpus = len(os.sched_getaffinity(0))
        ds = D.TrackNpzDataset(npz, _tracks(npz), track_length=TL, train=True, load_flow_data=True, load_primary_data=True)
        res = {}
        for rep in range(args.rounds):
            dl = torch.utils.data.DataLoader(ds, batch_size=BS, sampler=order, num_workers=4, drop_last=True, collate_fn=D.collate)
            n, s = _timed(dl)
            res.setdefault('npz_dataloader_w4', []).append(n * BS / s)
            for th in (1, 2, 4):
                ld = P.PackedTrackLoader(_tracks(packed), order, BS, TL, True, (H, W), primary=True, drop_last=True, num_threads=th,
                                         seed=rep, root=packed)
                n, s = _timed(ld)
                res.setdefault(f'packed_t{th}', []).append(n * BS / s)
        out = {'mode': 'host', 'cpus': cpus, 'imsize': [H, W], 'bs': BS, 'tracks_timed': args.tracks,
               'pinned': bool(torch.cuda.is_available()),
               'tracks_per_s': {k: [round(v, 1) for v in vs] for k, vs in res.items()}}
        ratio = min(res['packed_t4']) / max(res['npz_dataloader_w4'])
        out['packed_t4_over_npz_worst_case'] = round(ratio, 2)
        out['condition_4x'] = bool(ratio >= 4.0)
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(base, ignore_errors=True)


def e2e(args):
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam
    base = tempfile.mkdtemp(prefix='loader_rate_')
    try:
        npz, packed = make_roots(base, 16)
        wa = argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=TL, data_type='synthetic', architecture='multi_frame',
                                epochs=1, warmup_epochs=150, train_batch_size=BS, max_disp=128)
        skip = 4
        legs = {}
        for name, root in (('a_npz', npz), ('b_packed', packed)):
            w = multi_frame_worker.Worker(wa, data_root=root, num_workers=4, use_graph=True)
            w.current_epoch = 2
            w.get_test_sets()    # (builds the loss objects)
            torch.manual_seed(0)
            net = multi_frame_networks.FuseNet(imsize=w.imsizes[0], K=w.K, baseline=w.baseline, track_length=TL, max_disp=128).cuda()
            opt = FlatAdam(net.parameters(), lr=1e-4)
            ds = w.get_train_set()
            ds.sample_paths = _tracks(root) * (-(-(args.steps + skip + 1) * BS // 16))     # cycled
            legs[name] = (w, net, opt, ds)

        def run_loader_leg(name, epoch, steps):
            w, net, opt, ds = legs[name]
            if name == 'a_npz':
                from depthinspace_amd.model.worker import ShardSampler
                nw = w.num_workers
                loader = torch.utils.data.DataLoader(ds, batch_size=BS, sampler=ShardSampler(len(ds), 0, 1, True, w.seed, epoch),
                                                     num_workers=nw, drop_last=True, pin_memory=True, collate_fn=D.collate,
                                                     worker_init_fn=_seed_worker, multiprocessing_context='spawn' if nw else None)
            else:
                loader = w._loader(ds, BS, True, epoch)
            n, t0, graphed = 0, None, None
            for k, data in enumerate(loader):
                if k == skip:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if k >= skip + steps:
                    break
                graphed = w._graphed_step(net, opt, data)
                packed_b = data if hasattr(data, 'assemble') else None
                extra = {} if packed_b is not None else dict(data)
                extra['_aug_params'], extra['_aug_seed'] = w.draw_aug(BS * TL)
                graphed.run(extra, packed=packed_b)
                n += k >= skip
            torch.cuda.synchronize()
            dt = time.perf_counter() - (t0 if t0 is not None else 0.0)
            del loader
            return n * BS * TL / dt, graphed

        # warm-up: capture both steps once.  The .npz leg captures from an in-process loader: the pin-memory thread of a DataLoader with
        # worker processes allocates pinned memory while the main thread captures, which invalidates the capture
        # (hipErrorStreamCaptureInvalidated); the packed loader's threads make no HIP calls
        for name in legs:
            w = legs[name][0]
            keep, w.num_workers = w.num_workers, (0 if name == 'a_npz' else w.num_workers)
            run_loader_leg(name, 0, 0)     # (`skip` untimed steps)
            w.num_workers = keep
        res = {'a_npz': [], 'b_packed': [], 'c_resident': []}
        for r in range(args.rounds):
            for name in ('a_npz', 'b_packed'):
                fps, graphed = run_loader_leg(name, r + 1, args.steps)
                res[name].append(fps)
            for _ in range(skip):
                graphed.run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                graphed.run()
            torch.cuda.synchronize()
            res['c_resident'].append(args.steps * BS * TL / (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'mode': 'e2e', 'imsize': [H, W], 'bs': BS, 'steps_timed': args.steps, 'cpus': len(os.sched_getaffinity(0)),
                          'step_mode': graphed.mode, 'frames_per_s': {k: [round(x, 1) for x in v] for k, v in res.items()},
                          'b_over_a': round(med['b_packed'] / med['a_npz'], 3), 'b_over_c': round(med['b_packed'] / med['c_resident'], 3),
                          'b_beyond_spread_of_a': bool(min(res['b_packed']) > max(res['a_npz']))}), flush=True)
    finally:
        shutil.rmtree(base, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['host', 'e2e'])
    ap.add_argument('--tracks', type=int, default=64)
    ap.add_argument('--steps', type=int, default=44)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    (host if a.mode == 'host' else e2e)(a)
