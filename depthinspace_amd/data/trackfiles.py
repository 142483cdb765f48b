"""What the track tools (data/fuse.py, mesh.py, presave_sgm.py, presave_flow.py, presave_pose.py) share on the host: which disparities
of a track directory a `--disp` source names, the atomic npz writer, and the one-line report."""
import os

import numpy as np

SOURCES = ('gt', 'sgm', 'single_frame', 'multi_frame')


def _maps(a):
    """(tl, H, W) or (tl, 1, H, W) -> contiguous float32 (tl, H, W)"""
    return np.ascontiguousarray(a, dtype=np.float32).reshape((a.shape[0],) + a.shape[-2:])


def load_disp(d, source):
    """the disparities (tl, H, W) float32 of one track: `disp` (gt) or `sgm_disp` (sgm) of frames.npz, or the `disp` of
    single_frame_disp.npz / multi_frame_disp.npz"""
    if source not in SOURCES:
        raise ValueError(f'--disp is one of {SOURCES}')
    if source in ('gt', 'sgm'):
        path, key = os.path.join(d, 'frames.npz'), 'disp' if source == 'gt' else 'sgm_disp'
        with np.load(path) as f:
            if key not in f.files:
                raise ValueError(f'{d}/frames.npz has no array `{key}`')
            return _maps(f[key])
    path = os.path.join(d, f'{source}_disp.npz')
    if not os.path.exists(path):
        raise ValueError(f'{path} is missing (data/presave_disp.py writes it)')
    with np.load(path) as f:
        return _maps(f['disp'])


def load_track(d, source):
    """-> disp (tl, H, W), R (tl, 3, 3), t (tl, 3), ambient (tl, H, W), gt disp (tl, H, W) or None: float32 numpy"""
    if source not in SOURCES:
        raise ValueError(f'--disp is one of {SOURCES}')
    with np.load(os.path.join(d, 'frames.npz')) as f:
        R, t, amb = f['R'], f['t'], f['ambient']
        gt = _maps(f['disp']) if 'disp' in f.files else None
    return load_disp(d, source), np.ascontiguousarray(R, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32), _maps(amb), gt


def write_npz(path, arrays):
    """the dict `arrays` -> path, through a temporary file and os.replace: the file is the old one or the new one, never a part"""
    tmp = path + '.tmp.npz'   # (np.savez appends .npz to any other ending)
    try:
        np.savez(tmp, **arrays)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def rewrite_npz(path, extra):
    """the npz file at path plus (or with other) arrays `extra`: its other arrays are copied as they are"""
    with np.load(path) as f:
        arrays = {k: f[k] for k in f.files}
    arrays.update(extra)
    write_npz(path, arrays)


def report_text(res, fmt):
    """`key value` of the dict res, two spaces between: a float in the format `fmt`, anything else as it prints"""
    return '  '.join(f'{k} {v:{fmt}}' if isinstance(v, float) else f'{k} {v}' for k, v in res.items())
