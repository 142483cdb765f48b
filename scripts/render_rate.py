"""Rates of the track renderer (profiles/render_rate.md): tracks/s of dis_render_track by HIP events, next to the host generator.

    python scripts/render_rate.py [--h 512 --w 432 --tl 4 --scenes 8 --calls 24 --repeats 5] [--host-procs 16] [--out FILE]

sampled   scenes of data.render.sample_track (procedural library, default tessellation), uploaded before the clock starts
dense     one 65 536-triangle scene (three 20 480-face icospheres, a 4 094-face torus, the board)
hidden    the same triangle count with every object moved 4 m sideways, out of the camera's and the projector's view but in front
          of the near distance: the box walk without the ray tests
host      synth.make_batch(bs = 1) at the same size in --host-procs processes (the generator the renderer stands next to)
"""
import argparse
import itertools
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rate_common as RC   # noqa: E402


def dense_scene(hidden=False):
    from depthinspace_amd.data import meshes, render
    rng = np.random.RandomState(0)
    parts = [render.board(4.0)]
    for k, xy in enumerate(((-0.5, -0.4), (0.45, 0.5), (0.3, -0.6))):
        v, f = meshes.icosphere(5)
        parts.append((v * (0.5 + 0.1 * k) @ render.random_rotation(rng).T + np.array([xy[0], xy[1], 2.0 + 0.4 * k]), f))
    v, f = meshes.torus(segments=89, sides=23)
    parts.append((v * 0.8 @ render.random_rotation(rng).T + np.array([-0.3, 0.5, 1.6]), f))
    if hidden:
        parts = parts[:1] + [(v + np.array([4.0, 0.0, 0.0]), f) for v, f in parts[1:]]
    verts, faces = meshes.stack(parts)
    assert len(faces) == 65536
    albedo = np.full(len(faces), 0.7, np.float32)
    R, t, blend = render.sample_poses(rng, 4)
    return verts.astype(np.float32), faces.astype(np.int32), albedo, R, t, blend


def _host_track(seed):
    from depthinspace_amd import synth
    synth.make_batch(_host_track.settings, 1, _host_track.tl, seed=seed)
    return seed


def _host_init(h, w, tl):
    from depthinspace_amd import synth
    _host_track.settings = synth.make_settings(h, w)
    _host_track.tl = tl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--scenes', type=int, default=8)
    ap.add_argument('--calls', type=int, default=24)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-procs', type=int, default=16, help='0: skip the host generator')
    ap.add_argument('--host-tracks', type=int, default=64)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from depthinspace_amd import ops, synth
    from depthinspace_amd.data import meshes, render
    if not torch.cuda.is_available():
        sys.exit('render_rate: no GPU; a rate is measured on the device or not at all')
    dev = torch.device('cuda')
    settings = synth.make_settings(a.h, a.w)
    pattern = torch.from_numpy(np.ascontiguousarray(settings.pattern[..., 0])).to(dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    objs = meshes.default_objects()
    result = {'device': torch.cuda.get_device_name(0), 'h': a.h, 'w': a.w, 'tl': a.tl, 'calls': a.calls, 'repeats': a.repeats}

    def rate(scenes):
        dscenes = [tuple(up(x) for x in s[:5]) + (s[5],) for s in scenes]
        nf = max(len(s[1]) for s in scenes)
        ws = torch.empty(ops.lib.fn('dis_render_workspace')(max(len(s[0]) for s in scenes), nf, a.tl, a.h, a.w), dtype=torch.uint8, device=dev)
        run = lambda s: ops.render_track(s[0], s[1], s[2], s[3], s[4], settings.K, settings.baseline, s[5], pattern, want_ids=False, workspace=ws)
        for s in dscenes:
            run(s)
        torch.cuda.synchronize()
        turn = itertools.cycle(dscenes)
        rates = [1e3 / ms for ms in RC.windows(lambda: run(next(turn)), a.repeats, a.calls)[0]]
        return {'tracks_per_s': sorted(rates), 'median': float(np.median(rates)), 'faces': [len(s[1]) for s in scenes]}

    result['sampled'] = rate([render.sample_track(i, a.tl, 0, objs) for i in range(a.scenes)])
    result['dense'] = rate([dense_scene()])
    result['hidden'] = rate([dense_scene(hidden=True)])
    if a.host_procs > 0:
        with mp.get_context('spawn').Pool(a.host_procs, initializer=_host_init, initargs=(a.h, a.w, a.tl)) as pool:
            pool.map(_host_track, range(a.host_procs))          # start-up and imports outside the clock
            t0 = time.perf_counter()
            pool.map(_host_track, range(a.host_tracks), chunksize=1)
            result['host'] = {'procs': a.host_procs, 'tracks_per_s': a.host_tracks / (time.perf_counter() - t0)}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as fp:
            fp.write(line + '\n')


if __name__ == '__main__':
    main()
