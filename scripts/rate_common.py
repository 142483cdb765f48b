"""What the scripts/*_rate.py share: the timing arguments, the windows of calls between two HIP events, the same call captured into a
hipGraph on a side stream and replayed in the same windows, the result keys of both, and the JSON writer.  (torch is imported when a
measurement starts: the scripts parse their arguments without it.)"""
import json
import statistics

HBM_BYTES_PER_S = 8e12


def add_timing_args(ap, warmup=3, repeats=9, calls=50):
    ap.add_argument('--warmup', type=int, default=warmup)
    ap.add_argument('--repeats', type=int, default=repeats)
    ap.add_argument('--calls', type=int, default=calls)
    ap.add_argument('--json', default=None, help='also write the result lines to this file')


def windows(fn, repeats, calls, skip_first=False):
    """`repeats` windows of `calls` calls of fn, each between two HIP events -> (ms per call of every window, the last result);
    skip_first: one more window first, left out as the warm-up"""
    import torch
    ms, r = [], None
    for k in range(repeats + (1 if skip_first else 0)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        if k or not skip_first:
            ms.append(e0.elapsed_time(e1) / calls)
    return ms, r


def eager(call, warmup, repeats, calls):
    """`warmup` untimed calls, then the windows -> (ms per call of every window, the last result)"""
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    return windows(call, repeats, calls)


def replayed(call, repeats, calls):
    """the call captured once into a hipGraph on a side stream and replayed in the same windows, the first one dropped -> (ms per replay
    of every window, the captured call's result)"""
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call()
    return windows(graph.replay, repeats, calls, skip_first=True)[0], out


def time_call(call, warmup, repeats, calls):
    """-> the eager window times, the replay window times (ms per call), the last eager result, the captured result"""
    ms, r = eager(call, warmup, repeats, calls)
    gms, rg = replayed(call, repeats, calls)
    return ms, gms, r, rg


def ms_fields(prefix, ms):
    return {f'{prefix}_median': round(statistics.median(ms), 4), f'{prefix}_min': round(min(ms), 4), f'{prefix}_max': round(max(ms), 4)}


def timing_fields(n, ms, gms):
    """n tracks per call -> call_ms_*, tracks_per_s, graph_ms_*, graph_tracks_per_s"""
    return {**ms_fields('call_ms', ms), 'tracks_per_s': round(n / statistics.median(ms) * 1e3, 1),
            **ms_fields('graph_ms', gms), 'graph_tracks_per_s': round(n / statistics.median(gms) * 1e3, 1)}


def emit(lines, path):
    """the result lines (a list, or the one dict of a script with one result) -> the file --json names, if it names one"""
    if path:
        with open(path, 'w') as fp:
            json.dump(lines, fp, indent=1)
