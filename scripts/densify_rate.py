"""Rate of ops.disp_densify (csrc/densify.hip) on the MI355X next to the ops.sgm_disparity and ops.speckle_filter calls whose output it
takes, timed in the same job: rendered mesh-scene frames at 512 x 432, n = 4 and 16, ndisp 64, speckle 100 / 1.0, then gap 16, 6
directions, spread 2.0 (profiles/densify_rate.md).

Per n: n / 4 tracks of data/render.py are rendered, matched and speckle-filtered; then, for the matcher, the speckle filter and each form
of the densifier - the fill alone, the median alone with r = 1 and r = 2, both stages with r = 1 (the full post-filter) and with r = 2 -
`--warmup` untimed calls and `--repeats` windows of `--calls` calls each, every window between two HIP events, and the same call captured
into a hipGraph and replayed in the same windows; the median window gives the call time.  The achieved GB/s is the byte model below over
that time: a whole-call rate, not a kernel's share of the memory bandwidth.

Byte model of one call (N = n h w pixels; what the algorithm has to move if every array crossed the memory once per launch that uses it):
    fill      reads  N 4 (disp)                      writes N 4 (the map) + N (state)
    median    reads  N 4 (the fill's map, or disp)   writes N 4 (out) [+ N (state) when it runs alone]
The halos that the tiles read again (a tile of 64 x 16 with a halo of 16 stages 96 x 48 cells, 4.5 times its own) are not in the model;
they come from the L2.

    python scripts/densify_rate.py [--h 512 --w 432] [--n 4 16] [--gap 16] [--dirs 6] [--spread 2.0] [--check] [--warmup 5] [--repeats 15]
                                   [--calls 10] [--json PATH]
--check also compares out and state of every form at the first n with the numpy restatement tests/densify_ref.py.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rate_common as RC   # noqa: E402


def byte_model(n, h, w, gap, r):
    N = n * h * w
    fill = gap > 0 or r == 0
    return (N * 9 if fill else 0) + ((N * 8 if fill else N * 9) if r > 0 else 0)


def quality(disp, truth):
    """the valid pixels (disp != 0 where the surface was seen), and of those the counts more than 0.5, 1 and 5 px off"""
    ok = (disp != 0) & (truth > 0)
    err = (disp - truth).abs()
    return [int(ok.sum())] + [int(((err > t) & ok).sum()) for t in (0.5, 1, 5)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=432)
    ap.add_argument('--n', type=int, nargs='+', default=[4, 16], help='frames per call, a multiple of 4 (tracks of 4 frames are rendered)')
    ap.add_argument('--ndisp', type=int, default=64)
    ap.add_argument('--max-size', type=int, default=100)
    ap.add_argument('--max-diff', type=float, default=1.0)
    ap.add_argument('--gap', type=int, default=16)
    ap.add_argument('--dirs', type=int, default=6)
    ap.add_argument('--spread', type=float, default=2.0)
    ap.add_argument('--seed', type=int, default=11)
    ap.add_argument('--check', action='store_true', help='compare the first n with tests/densify_ref.py')
    RC.add_timing_args(ap, warmup=5, repeats=15, calls=10)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from depthinspace_amd import lib, ops, synth
    from depthinspace_amd.data import render
    if not torch.cuda.is_available():
        raise SystemExit('densify_rate.py measures on the GPU: no device found')
    st = synth.make_settings(a.h, a.w)
    pat = torch.from_numpy(np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)).cuda()
    forms = [('fill', a.gap, 0), ('median_r1', 0, 1), ('median_r2', 0, 2), ('fill_median_r1', a.gap, 1), ('fill_median_r2', a.gap, 2)]
    lines = []
    for k, n in enumerate(a.n):
        if n % 4:
            raise SystemExit('--n: multiples of 4')
        batch = render.render_batch(st, n // 4, tl=4, seed=a.seed)
        im = batch['im0'].reshape(n, 1, a.h, a.w).contiguous()
        truth = batch['disp0'].reshape(n, 1, a.h, a.w)
        ws_m = torch.empty(lib.fn('dis_sgm_workspace')(n, a.h, a.w, a.ndisp), dtype=torch.uint8, device='cuda')
        ws_f = torch.empty(lib.fn('dis_speckle_workspace')(n, a.h, a.w), dtype=torch.uint8, device='cuda')
        ws_d = torch.empty(lib.fn('dis_disp_densify_workspace')(n, a.h, a.w), dtype=torch.uint8, device='cuda')
        m_ms, m_gms, sgm, _ = RC.time_call(lambda: ops.sgm_disparity(im, pat, ndisp=a.ndisp, workspace=ws_m), a.warmup, a.repeats, a.calls)
        f_ms, f_gms, flt, _ = RC.time_call(lambda: ops.speckle_filter(sgm, a.max_size, a.max_diff, workspace=ws_f), a.warmup, a.repeats,
                                           a.calls)
        m_med = statistics.median(m_ms)
        res = {'h': a.h, 'w': a.w, 'n': n, 'ndisp': a.ndisp, 'max_size': a.max_size, 'max_diff': a.max_diff, 'gap': a.gap, 'dirs': a.dirs,
               'spread': a.spread, **RC.ms_fields('matcher_call_ms', m_ms), **RC.ms_fields('matcher_graph_ms', m_gms),
               **RC.ms_fields('speckle_call_ms', f_ms), **RC.ms_fields('speckle_graph_ms', f_gms),
               'workspace_bytes': int(ws_d.numel()), 'holes_share': round(float((flt == 0).float().mean()), 4), 'quality_keys':
               ['valid', 'off_by_more_than_0.5px', 'off_by_more_than_1px', 'off_by_more_than_5px'], 'quality_speckle': quality(flt, truth)}
        for name, gap, r in forms:
            call = lambda: ops.disp_densify(flt, gap, a.dirs, a.spread, r, workspace=ws_d)   # noqa: E731
            d_ms, d_gms, out, out_g = RC.time_call(call, a.warmup, a.repeats, a.calls)
            assert torch.equal(out.view(torch.int32), out_g.view(torch.int32))
            d_med = statistics.median(d_ms)
            model = byte_model(n, a.h, a.w, gap, r)
            res[name] = {**RC.ms_fields('call_ms', d_ms), **RC.ms_fields('graph_ms', d_gms), 'over_matcher': round(d_med / m_med, 4),
                         'frames_per_s': round(n / d_med * 1e3, 1), 'model_bytes': model, 'achieved_GB_per_s': round(model / d_med / 1e6, 1),
                         'quality': quality(out, truth)}
            if gap > 0:
                _, state = ops.disp_densify(flt, gap, a.dirs, a.spread, r, want_state=True, workspace=ws_d)
                res[name]['filled'] = int((state == 2).sum())
            if a.check and k == 0:
                from tests import densify_ref
                out, state = ops.disp_densify(flt, gap, a.dirs, a.spread, r, want_state=True, workspace=ws_d)
                want, want_state = densify_ref.disp_densify(flt.cpu().numpy(), gap, a.dirs, a.spread, r)
                res[name]['equals_restatement'] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and
                                                       np.array_equal(state.cpu().numpy(), want_state))
        print(json.dumps(res))
        lines.append(res)
    RC.emit(lines, a.json)


if __name__ == '__main__':
    main()
