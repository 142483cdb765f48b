"""GPU, end to end: rendered tracks on disk -> data/presave_sgm.py (ops.sgm_disparity) -> the `real` reader -> the warm-up term
ops.sgm_l1.  The camera's baseline is 16 times the default one, so that the board itself (z in [3, 5], fx * baseline = 174) lies
beyond the 30-pixel threshold of the warm-up mask; 256 candidates cover every surface farther than 0.68."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import sgm_ref

pytestmark = pytest.mark.gpu

H, W, NDISP = 32, 256, 256


def test_presave_report_and_warmup_term(tmp_path, capsys):
    from depthinspace_amd import ops, synth
    from depthinspace_amd.data import dataset as D, presave_sgm as P, render
    st = synth.make_settings(H, W)
    st.baseline = 0.4
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    # 1. presave with the report
    res = P.presave_sgm(root, ndisp=NDISP, report=True)
    line = capsys.readouterr().out
    assert 'valid' in line and 'of1' in line
    ref_root = str(tmp_path / 'ref')
    shutil.copytree(root, ref_root)
    pat = np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)
    for p in paths:
        with np.load(os.path.join(p, 'frames.npz')) as f:
            sgm, im, truth = f['sgm_disp'], f['im'], f['disp']
        assert sgm.shape == (4, 1, H, W) and sgm.dtype == np.float32 and np.isfinite(sgm).all()
        assert truth.max() > 30 and (sgm > 30).any()
        # 2. the file holds the numpy reference's array, bit for bit
        want = sgm_ref.sgm_disparity(im[:, 0], pat, ndisp=NDISP)['disp'][:, None]
        assert np.array_equal(sgm, want)
        q = os.path.join(ref_root, os.path.basename(p), 'frames.npz')
        with np.load(q) as f:
            arrays = {k: f[k] for k in f.files}
        arrays['sgm_disp'] = want
        np.savez(q, **arrays)
    # 3. the baseline numbers: the report of the kernel's arrays against the report of the reference's (equal arrays, so the margin
    #    of half a percentage point covers nothing but the rounding of the metric)
    ref = P.sgm_report(ref_root)
    print(f'sgm baseline, 2 rendered tracks {H} x {W}, baseline 0.4, ndisp {NDISP}: ' + '  '.join(f'{k} {v:.4f}' for k, v in res.items()))
    assert 0 < res['valid'] <= 1 and np.isfinite(res['of1'])
    assert res['of1'] <= ref['of1'] + 0.005, (res, ref)
    assert res['valid'] == ref['valid']
    # incremental: a second call matches nothing
    assert P.presave_sgm(root, ndisp=NDISP) == 0
    # 4. the warm-up term on the loaded batch
    ds = D.TrackNpzDataset(root, paths, track_length=4, train=False, data_type='real')
    batch = D.collate([ds[0], ds[1]])
    sgm = batch['sgm_disp'].cuda()
    assert tuple(sgm.shape) == (2, 4, 1, H, W)
    mask = sgm > 30
    assert int(mask.sum()) > 0
    o = (batch['disp0'].cuda() + 0.3).requires_grad_(True)
    noise = torch.randn_like(sgm)
    loss = ops.sgm_l1(o, sgm, noise, 30.0)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0 and bool(torch.isfinite(o.grad).all())
    assert not bool(((o.grad != 0) & ~mask).any()) and int((o.grad != 0).sum()) > 0


def test_render_writes_sgm_disp_on_request(tmp_path):
    """write_rendered_dataset(sgm=N) stores what presave_sgm computes; without it the files have no such array"""
    from depthinspace_amd import synth
    from depthinspace_amd.data import presave_sgm as P, render
    st = synth.make_settings(32, 96)
    a = render.write_rendered_dataset(str(tmp_path / 'a'), st, 1, seed=2, sgm=64)
    b = render.write_rendered_dataset(str(tmp_path / 'b'), st, 1, seed=2)
    with np.load(os.path.join(b[0], 'frames.npz')) as f:
        assert sorted(f.files) == ['R', 'ambient', 'disp', 'grad', 'im', 't']
    assert P.presave_sgm(str(tmp_path / 'a')) == 0 and P.presave_sgm(str(tmp_path / 'b')) == 1
    with np.load(os.path.join(a[0], 'frames.npz')) as fa, np.load(os.path.join(b[0], 'frames.npz')) as fb:
        assert sorted(fa.files) == sorted(fb.files)
        for k in fa.files:
            assert np.array_equal(fa[k], fb[k]), k
