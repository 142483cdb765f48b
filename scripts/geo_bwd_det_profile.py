"""Backward of the flow-consistency loss at the training step's shape, order-free (dis_geo_loss_bwd_multi_det) against atomic
(dis_geo_loss_bwd_multi): 12 directional terms, bs 4, 512 x 432, inputs of tests/pixel_ref.py::geo_input.  HIP events around 10 calls
of one form, the two forms alternating, median of 7 rounds - the numbers of profiles/geo_bwd_det.md.

    python scripts/geo_bwd_det_profile.py [--bs 4] [--h 512] [--w 432] [--tl 4] [--mode mf|sf]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from depthinspace_amd import lib, ops
from tests import pixel_ref as P

ROUNDS, CALLS = 7, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=4)
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--tl', type=int, default=4)
    ap.add_argument('--mode', default='mf', choices=['mf', 'sf'])
    a = ap.parse_args()
    bs, h, w, tl = a.bs, a.h, a.w, a.tl
    g = P.geo_input(bs, h, w, tl=tl)
    pairs = [(i, j) for i in range(tl) for j in range(tl) if i != j]
    T = len(pairs)
    K, Ki = lib.host_floats(g['K'].reshape(-1)), lib.host_floats(g['Kinv'].reshape(-1))
    clamp = P.GEO_CLAMP if a.mode == 'sf' else -1.0
    depth, amb, R, t = g['depth'].cuda(), g['amb'].cuda(), g['R'].cuda(), g['t'].cuda()
    pdepth = g['pdepth'].cuda() if a.mode == 'mf' else None
    f0 = [g['flow'][p].cuda() for p in pairs]
    f1 = [g['flow'][(j, i)].cuda() for (i, j) in pairs]
    mask = torch.empty((T, bs, 1, h, w), dtype=torch.float32).cuda()
    acc = torch.empty(lib.fn('dis_geo_loss_multi_acc_doubles')(T), dtype=torch.float64).cuda()
    out = torch.empty(T, dtype=torch.float32).cuda()
    tab = ops._GeoLossAll._table(pairs, depth, R, t, mask, f0, f1, amb, pdepth)
    lib.call('dis_geo_loss_fwd_multi', tab, T, K, Ki, clamp, acc, out, bs, h, w)
    gd = torch.zeros_like(depth)
    tab = ops._GeoLossAll._table(pairs, depth, R, t, mask, f0, gdepth=gd)
    gscale = torch.full((T,), 0.2 / (T / 2), dtype=torch.float32).cuda()
    nbytes = lib.fn('dis_geo_loss_bwd_det_workspace')(T, bs, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8).cuda()

    def atomic():
        lib.call('dis_geo_loss_bwd_multi', tab, T, K, Ki, clamp, acc, gscale, bs, h, w)

    def det():
        lib.call('dis_geo_loss_bwd_multi_det', tab, T, K, Ki, clamp, acc, gscale, bs, h, w, ws)

    forms = (('atomic', atomic), ('det', det))
    for _, f in forms:   # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in forms}
    for _ in range(ROUNDS):
        for n, f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                f()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1) / CALLS)
    print(f'mask share {float(mask.mean()):.3f}  terms {T}  bs {bs}  {h} x {w}  {a.mode}  workspace {nbytes} bytes ({nbytes / 2 ** 20:.1f} MiB)')
    for n, _ in forms:
        v = ms[n]
        print(f'{n:7s} median {statistics.median(v) * 1e3:8.1f} us per call   min {min(v) * 1e3:8.1f}   max {max(v) * 1e3:8.1f}   '
              f'({ROUNDS} rounds of {CALLS} calls)')
    taps = 4 * 8 * float(mask.sum())   # an upper bound: valid taps of unclamped masked-in pixels, 8 bytes each
    print(f'det / atomic {statistics.median(ms["det"]) / statistics.median(ms["atomic"]):.2f}   '
          f'8-byte integer atomics: <= {taps / 1e6:.1f} MB added per call')


if __name__ == '__main__':
    main()
