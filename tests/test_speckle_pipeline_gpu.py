"""GPU, end to end: rendered tracks on disk -> data/presave_sgm.py --speckle (ops.sgm_disparity, then ops.speckle_filter) -> --report.
The dataset is that of tests/test_sgm_pipeline_gpu.py: two tracks at 32 x 256, baseline 0.4, 256 candidates, seed 11; the second track
has objects nearer than the candidate range reaches, where the matcher mostly fails and leaves islands."""
import os
import shutil
import zipfile

import numpy as np
import pytest

from tests import sgm_ref, speckle_ref

pytestmark = pytest.mark.gpu

H, W, NDISP = 32, 256, 256


def _members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i.filename)) for i in z.infolist()]


def test_presave_with_speckle_report_and_refilter(tmp_path, capsys):
    from depthinspace_amd import synth
    from depthinspace_amd.data import presave_sgm as P, render
    st = synth.make_settings(H, W)
    st.baseline = 0.4
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    raw_root = str(tmp_path / 'raw')
    shutil.copytree(root, raw_root)
    # 1. matched and filtered in one go: the file holds the restatement of the filter on the restatement of the matcher, bit for bit
    assert P.presave_sgm(root, ndisp=NDISP, speckle=100) == 2
    pat = np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)
    removed = 0
    for p in paths:
        with np.load(os.path.join(p, 'frames.npz')) as f:
            sgm, im = f['sgm_disp'], f['im']
        assert sgm.shape == (4, 1, H, W) and sgm.dtype == np.float32
        matched = sgm_ref.sgm_disparity(im[:, 0], pat, ndisp=NDISP)['disp'][:, None].astype(np.float32)
        want = speckle_ref.speckle_filter(matched, 100, 1.0)[0]
        assert np.array_equal(sgm.view(np.uint32), want.view(np.uint32))
        removed += int(((matched != 0) & (sgm == 0)).sum())
    assert removed > 0
    # 2. the report against that of an unfiltered copy, over both tracks
    assert P.presave_sgm(raw_root, ndisp=NDISP) == 2
    raw = P.sgm_report(raw_root)
    res = P.presave_sgm(root, ndisp=NDISP, speckle=100, report=True)
    assert 'of5' in capsys.readouterr().out
    print(f'2 rendered tracks {H} x {W}, baseline 0.4, ndisp {NDISP}: unfiltered ' + '  '.join(f'{k} {v:.4f}' for k, v in raw.items()))
    print('filtered with size 100, diff 1.0: ' + '  '.join(f'{k} {v:.4f}' for k, v in res.items()))
    print(f'of5 ratio {res["of5"] / raw["of5"]:.4f}, valid ratio {res["valid"] / raw["valid"]:.4f}')
    assert res['valid'] > 0
    assert res['of5'] <= 0.5 * raw['of5'], (res, raw)
    # 3. the round trip: matching without the filter, then --refilter, gives the same files
    before = [_members(os.path.join(raw_root, os.path.basename(p), 'frames.npz')) for p in paths]
    assert P.presave_sgm(raw_root, ndisp=NDISP, speckle=100, refilter=True) == 2
    for p, old in zip(paths, before):
        q = os.path.join(raw_root, os.path.basename(p))
        assert sorted(os.listdir(q)) == sorted(os.listdir(p))
        assert _members(os.path.join(q, 'frames.npz')) == _members(os.path.join(p, 'frames.npz'))
        now = _members(os.path.join(q, 'frames.npz'))
        assert [m for m in now if m[0] != 'sgm_disp.npy'] == [m for m in old if m[0] != 'sgm_disp.npy']
    # idempotent: nothing is left to filter, no file is written
    stamps = [os.stat(os.path.join(raw_root, os.path.basename(p), 'frames.npz')).st_mtime_ns for p in paths]
    assert P.presave_sgm(raw_root, ndisp=NDISP, speckle=100, refilter=True) == 0
    assert [os.stat(os.path.join(raw_root, os.path.basename(p), 'frames.npz')).st_mtime_ns for p in paths] == stamps
