"""GPU, end to end: rendered tracks on disk -> data/presave_sgm.py --speckle --fill --median (ops.sgm_disparity, ops.speckle_filter, then
ops.disp_densify) -> --report.  The dataset is that of tests/test_speckle_pipeline_gpu.py: two tracks at 32 x 256, baseline 0.4, 256
candidates, seed 11.  No quality bar is set on it: the lines it prints are the ones DESIGN.md section 7 quotes."""
import os
import shutil
import zipfile

import numpy as np
import pytest

from tests import densify_ref, sgm_ref, speckle_ref

pytestmark = pytest.mark.gpu

H, W, NDISP = 32, 256, 256
STAGES = dict(speckle=100, fill=16, median=1)


def _members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i.filename)) for i in z.infolist()]


def test_presave_with_fill_and_median_report_and_refilter(tmp_path, capsys):
    from depthinspace_amd import synth
    from depthinspace_amd.data import presave_sgm as P, render
    st = synth.make_settings(H, W)
    st.baseline = 0.4
    root = str(tmp_path / 'data')
    paths = render.write_rendered_dataset(root, st, 2, seed=11)
    raw_root, speckle_root = str(tmp_path / 'raw'), str(tmp_path / 'speckle')
    shutil.copytree(root, raw_root)
    shutil.copytree(root, speckle_root)
    # 1. all stages in one go: the file holds the three restatements chained on the host, bit for bit
    assert P.presave_sgm(root, ndisp=NDISP, **STAGES) == 2
    pat = np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)
    filled = 0
    for p in paths:
        with np.load(os.path.join(p, 'frames.npz')) as f:
            sgm, state, im = f['sgm_disp'], f['sgm_state'], f['im']
        assert sgm.shape == (4, 1, H, W) and sgm.dtype == np.float32 and state.shape == (4, 1, H, W) and state.dtype == np.uint8
        matched = sgm_ref.sgm_disparity(im[:, 0], pat, ndisp=NDISP)['disp'][:, None].astype(np.float32)
        want, want_state = densify_ref.disp_densify(speckle_ref.speckle_filter(matched, 100, 1.0)[0], 16, 6, 2.0, 1)
        assert np.array_equal(sgm.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(state[:, 0], want_state)
        filled += int((state == 2).sum())
    assert filled > 0
    # 2. the report beside that of a speckle-only copy, over both tracks
    assert P.presave_sgm(speckle_root, ndisp=NDISP, speckle=100) == 2
    only = P.sgm_report(speckle_root)
    capsys.readouterr()
    res = P.presave_sgm(root, ndisp=NDISP, report=True, **STAGES)
    line = capsys.readouterr().out
    assert 'filled' in line and 'of1_filled' in line and 'of5' in line
    with capsys.disabled():                              # (the lines DESIGN.md quotes: shown whether the test passes or not)
        print(f'\n2 rendered tracks {H} x {W}, baseline 0.4, ndisp {NDISP}, speckle 100 / 1.0: ' +
              '  '.join(f'{k} {v:.4f}' for k, v in only.items()))
        print('then fill 16 / 6 / 2.0 and the 3 x 3 median: ' + '  '.join(f'{k} {v:.4f}' for k, v in res.items()))
    assert 'filled' not in only and 0 < res['filled'] < 1 and 0 <= res['of1_filled'] <= 1
    assert res['valid'] > only['valid'], (res, only)
    # 3. the round trip: matching without any filter, then --refilter with the same options, gives the same files
    assert P.presave_sgm(raw_root, ndisp=NDISP) == 2
    before = [_members(os.path.join(raw_root, os.path.basename(p), 'frames.npz')) for p in paths]
    assert P.presave_sgm(raw_root, ndisp=NDISP, refilter=True, **STAGES) == 2
    for p, old in zip(paths, before):
        q = os.path.join(raw_root, os.path.basename(p))
        assert sorted(os.listdir(q)) == sorted(os.listdir(p))
        now = _members(os.path.join(q, 'frames.npz'))
        assert now == _members(os.path.join(p, 'frames.npz'))
        assert [m for m in now if m[0] not in ('sgm_disp.npy', 'sgm_state.npy')] == [m for m in old if m[0] != 'sgm_disp.npy']
    # 4. a second --refilter writes nothing: the tracks store sgm_state and are final
    stamps = [os.stat(os.path.join(raw_root, os.path.basename(p), 'frames.npz')).st_mtime_ns for p in paths]
    capsys.readouterr()
    assert P.presave_sgm(raw_root, ndisp=NDISP, refilter=True, **STAGES) == 0
    assert '2 tracks' in capsys.readouterr().out
    assert [os.stat(os.path.join(raw_root, os.path.basename(p), 'frames.npz')).st_mtime_ns for p in paths] == stamps
