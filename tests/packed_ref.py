"""numpy reference of the packed-track batch assembly (what dis_assemble_tracks computes), and helpers shared by
tests/test_packed_loader_cpu.py and tests/test_packed_loader_gpu.py.  The reference indexes the arrays by name and frame - it
shares only record_layout() with the code under test."""
import os

import numpy as np

from depthinspace_amd.data import packed as P


def make_root(root, h, w, n, seed=50, sgm=False, primary=True, pseudo=True):
    """write_synthetic_dataset + the pre-saved disparities DIS-MF / DIS-FTSF read (copies of `disp`, offset so that the three
    differ) + an optional sgm_disp in frames.npz; returns the track directories"""
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D
    paths = D.write_synthetic_dataset(str(root), synth.make_settings(h, w), n, seed=seed)
    for d in paths:
        with np.load(os.path.join(d, 'frames.npz')) as f:
            fr = {k: f[k] for k in f.files}
        if sgm:
            fr['sgm_disp'] = (fr['disp'] * 0.5 + 3.0).astype(np.float32)
            np.savez(os.path.join(d, 'frames.npz'), **fr)
        if primary:
            np.savez(os.path.join(d, 'single_frame_disp.npz'), disp=(fr['disp'] + 1.0).astype(np.float32))
        if pseudo:
            np.savez(os.path.join(d, 'multi_frame_disp.npz'), disp=(fr['disp'] + 2.0).astype(np.float32))
    return paths


def split_record(rec, h, w, has_sgm, primary, pseudo):
    """one record (1-D float array) -> its arrays by name: im/ambient/disp/... (4,1,h,w), R, t, flow_ij (1,2,h,w)"""
    lay = P.record_layout(h, w, has_sgm, primary, pseudo)
    hw = h * w
    out = {}
    for k in ('im', 'ambient', 'disp', 'sgm_disp', 'primary_disp', 'pseudo_gt'):
        if k in lay:
            out[k] = rec[lay[k]:lay[k] + 4 * hw].reshape(4, 1, h, w)
    out['R'] = rec[lay['R']:lay['R'] + 36].reshape(4, 3, 3)
    out['t'] = rec[lay['t']:lay['t'] + 12].reshape(4, 3)
    for n, p in enumerate(P.PAIRS):
        out['flow_' + p] = rec[lay['flow'] + n * 2 * hw:lay['flow'] + (n + 1) * 2 * hw].reshape(1, 2, h, w)
    return out


_KEYS = {'im': 'im0', 'ambient': 'ambient0', 'disp': 'disp0', 'sgm_disp': 'sgm_disp', 'primary_disp': 'primary_disp',
         'pseudo_gt': 'pseudo_gt', 'R': 'R', 't': 't'}


def assemble(raw, stride, perm, h, w, has_sgm, primary, pseudo, want_sgm=None):
    """raw: 1-D float array holding record b at [b * stride:]; perm (bs, tl) -> {key: (tl, bs, ...)} plus '_flow_stacked'
    (tl * tl, bs, 2, h, w) with zero diagonal planes"""
    perm = np.asarray(perm)
    bs, tl = perm.shape
    want_sgm = has_sgm if want_sgm is None else want_sgm
    size = P.record_layout(h, w, has_sgm, primary, pseudo)['size']
    recs = [split_record(raw[b * stride:b * stride + size], h, w, has_sgm, primary, pseudo) for b in range(bs)]
    out = {}
    for k, key in _KEYS.items():
        if k not in recs[0] or (k == 'sgm_disp' and not want_sgm):
            continue
        out[key] = np.stack([np.stack([recs[b][k][perm[b][i]] for b in range(bs)]) for i in range(tl)])
    fs = np.zeros((tl * tl, bs, 2, h, w), np.float32)
    for i in range(tl):
        for j in range(tl):
            if i != j:
                for b in range(bs):
                    fs[i * tl + j, b] = recs[b][f'flow_{perm[b][i]}{perm[b][j]}'][0]
    out['_flow_stacked'] = fs
    return out


def collate_to_assembled(batch):
    """a `collate`d TrackNpzDataset batch ((bs, tl, ...) tensors, flow_ij (bs, 1, 2, h, w)) in the assembled layout"""
    out = {}
    tl = batch['im0'].shape[1]
    for k, v in batch.items():
        v = v.numpy()
        if not k.startswith('flow_'):
            out[k] = np.ascontiguousarray(np.swapaxes(v, 0, 1))
    bs, h, w = batch['im0'].shape[0], batch['im0'].shape[-2], batch['im0'].shape[-1]
    fs = np.zeros((tl * tl, bs, 2, h, w), np.float32)
    for i in range(tl):
        for j in range(tl):
            if i != j:
                fs[i * tl + j] = batch[f'flow_{i}{j}'].numpy()[:, 0]
    out['_flow_stacked'] = fs
    return out
