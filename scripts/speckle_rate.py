"""Rate of ops.speckle_filter (csrc/speckle.hip) on the MI355X next to the ops.sgm_disparity call whose output it filters, timed in the
same job: rendered mesh-scene frames at 512 x 432, n = 4 and 16, ndisp 64, max_size 100, max_diff 1.0 (profiles/speckle_rate.md).

Per n: n / 4 tracks of data/render.py are rendered and matched; then, for the matcher and for the filter, `--warmup` untimed calls and
`--repeats` windows of `--calls` calls each, every window between two HIP events, and the same call captured into a hipGraph and replayed
in the same windows; the median window gives the call time.  The achieved GB/s is the byte model below over that time: a whole-call
rate (four launches and the gaps between them), not a kernel's share of the memory bandwidth.

Byte model of one filter call (N = n h w pixels, P = n ((ceil(h / 16) - 1) w + (ceil(w / 64) - 1) h) pixel pairs across tile borders;
what the algorithm has to move if every array crossed the memory once per launch that uses it):
    tile      reads  N 4 (disp)                                     writes N 8 (parent, count)
    merge     reads  P 16 (the pair's disparities and the pair to its left) + P 8 (the two parents)   writes at most P 4 (atomic minima)
    flatten   reads  N 12 (parent, the root's parent, count)        writes N 4 (root)
    apply     reads  N 12 (disp, root, the root's count)            writes N 4 (out)
The chains of parents that merge and flatten walk are not in the model; they are what the times are made of.

    python scripts/speckle_rate.py [--h 512 --w 432] [--n 4 16] [--max-size 100] [--max-diff 1.0] [--check] [--warmup 5] [--repeats 15]
                                   [--calls 10] [--json PATH]
--check also compares out, label and size of the first n with the numpy restatement tests/speckle_ref.py (seconds of host time).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rate_common as RC   # noqa: E402

TILE_W, TILE_H = 64, 16    # csrc/speckle.hip


def byte_model(n, h, w):
    """-> dict launch -> bytes of one call"""
    N = n * h * w
    P = n * ((-(-h // TILE_H) - 1) * w + (-(-w // TILE_W) - 1) * h)
    return {'tile': N * 12, 'merge': P * 28, 'flatten': N * 16, 'apply': N * 16}


def quality(disp, truth):
    """the valid pixels (disp != 0 where the surface was seen), and of those the counts more than 1 and 5 px off"""
    ok = (disp != 0) & (truth > 0)
    err = (disp - truth).abs()
    return int(ok.sum()), int(((err > 1) & ok).sum()), int(((err > 5) & ok).sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--n', type=int, nargs='+', default=[4, 16], help='frames per call, a multiple of 4 (tracks of 4 frames are rendered)')
    ap.add_argument('--ndisp', type=int, default=64)
    ap.add_argument('--max-size', type=int, default=100)
    ap.add_argument('--max-diff', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=11)
    ap.add_argument('--check', action='store_true', help='compare the first n with tests/speckle_ref.py')
    RC.add_timing_args(ap, warmup=5, repeats=15, calls=10)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from depthinspace_amd.data import render
    if not torch.cuda.is_available():
        raise SystemExit('speckle_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    pat = torch.from_numpy(np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)).cuda()
    lines = []
    for k, n in enumerate(a.n):
        if n % 4:
            raise SystemExit('--n: multiples of 4')
        batch = render.render_batch(st, n // 4, tl=4, seed=a.seed)
        im = batch['im0'].reshape(n, 1, a.h, a.w).contiguous()
        truth = batch['disp0'].reshape(n, 1, a.h, a.w)
        ws_m = torch.empty(lib.fn('dis_sgm_workspace')(n, a.h, a.w, a.ndisp), dtype=torch.uint8, device='cuda')
        ws_f = torch.empty(lib.fn('dis_speckle_workspace')(n, a.h, a.w), dtype=torch.uint8, device='cuda')
        m_ms, m_gms, sgm, _ = RC.time_call(lambda: ops.sgm_disparity(im, pat, ndisp=a.ndisp, workspace=ws_m), a.warmup, a.repeats, a.calls)
        f_ms, f_gms, out, out_g = RC.time_call(lambda: ops.speckle_filter(sgm, a.max_size, a.max_diff, workspace=ws_f), a.warmup,
                                               a.repeats, a.calls)
        assert torch.equal(out.view(torch.int32), out_g.view(torch.int32))
        _, dbg = ops.speckle_filter(sgm, a.max_size, a.max_diff, want_debug=True, workspace=ws_f)
        torch.cuda.synchronize()
        ok = dbg['label'] >= 0
        roots = ok & (dbg['label'] == torch.arange(a.h * a.w, device='cuda', dtype=torch.int32).reshape(1, a.h, a.w))
        small = roots & (dbg['size'] <= a.max_size)
        model = byte_model(n, a.h, a.w)
        total = sum(model.values())
        f_med, m_med = statistics.median(f_ms), statistics.median(m_ms)
        v0, b1_0, b5_0 = quality(sgm, truth)
        v1, b1_1, b5_1 = quality(out, truth)
        res = {'h': a.h, 'w': a.w, 'n': n, 'ndisp': a.ndisp, 'max_size': a.max_size, 'max_diff': a.max_diff,
               **RC.ms_fields('filter_call_ms', f_ms), **RC.ms_fields('filter_graph_ms', f_gms),
               **RC.ms_fields('matcher_call_ms', m_ms), **RC.ms_fields('matcher_graph_ms', m_gms),
               'filter_over_matcher': round(f_med / m_med, 4), 'filter_frames_per_s': round(n / f_med * 1e3, 1),
               'model_bytes': total, 'model_bytes_by_launch': model, 'achieved_GB_per_s': round(total / f_med / 1e6, 1),
               'workspace_bytes': int(ws_f.numel()), 'components': int(roots.sum()), 'components_removed': int(small.sum()),
               'largest_component': int(dbg['size'].max()),
               'valid_pixels': [v0, v1], 'off_by_more_than_1px': [b1_0, b1_1], 'off_by_more_than_5px': [b5_0, b5_1],
               'share_off_by_more_than_5px': [round(b5_0 / max(v0, 1), 5), round(b5_1 / max(v1, 1), 5)]}
        if a.check and k == 0:
            from tests import speckle_ref
            want, label, size = speckle_ref.speckle_filter(sgm.cpu().numpy(), a.max_size, a.max_diff)
            res['equals_restatement'] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and
                                             np.array_equal(dbg['label'].cpu().numpy(), label) and
                                             np.array_equal(dbg['size'].cpu().numpy(), size))
        print(json.dumps(res))
        lines.append(res)
    RC.emit(lines, a.json)


if __name__ == '__main__':
    main()
