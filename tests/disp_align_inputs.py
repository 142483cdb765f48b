"""Inputs and cached restatements shared by the disparity-alignment tests (tests/test_disp_align_ref_cpu.py,
tests/test_disp_align_gpu.py): rendered tracks of tests/render_scenes.small_scene, their exact disparities, flows, ambient images and
poses from tests/render_ref (float64)."""
import numpy as np

from tests import disp_align_ref as DR
from tests.pose_inputs import pair_truth

# (n, tl, H, W): two levels; odd extents - the 2 x 2 blocks drop a row and a column -, two tracks of 6 pairs; three levels, all 12 pairs,
# several workgroups per image; one level, smaller than a tile in y
SHAPES = [(1, 2, 64, 48), (2, 3, 65, 51), (1, 4, 128, 96), (1, 2, 24, 40)]
KINDS = ['exact', 'holes', 'noise']
# of render_scenes.small_scene, one per track: seeds for which no pass of a float64 restatement has more than 4 borderline pixels
# (tests/test_disp_align_ref_cpu.py asserts it; at 128 x 96 the seeds 1 .. 3 have up to 6)
SEEDS = {SHAPES[0]: (1,), SHAPES[1]: (2, 3), SHAPES[2]: (6,), SHAPES[3]: (2,)}
MIN_CORR = 64
CASES = [(s, k) for s in SHAPES for k in KINDS]

_BASE, _INPUT, _REF, _FLOW = {}, {}, {}, {}


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def case_id(c):
    return f'{shape_id(c[0])}-{c[1]}'


def _render(shape):
    if shape not in _BASE:
        from tests import render_ref, render_scenes
        n, tl, H, W = shape
        s = render_scenes.small_settings(H, W)
        keys = ('disp', 'flow', 'ambient', 'visible_in')
        acc = {k: [] for k in keys + ('R', 't')}
        for seed in SEEDS[shape]:
            verts, faces, albedo, R, t, blend = render_scenes.small_scene(seed, tl)
            r = render_ref.render_ref(verts, faces, albedo, R, t, s.K, s.baseline, blend, s.pattern[..., 0], dtype=np.float64, ambiguity=False)
            for k, sh in zip(keys, ((tl, H, W), (tl * tl, 2, H, W), (tl, H, W), (tl * tl, H, W))):
                acc[k].append(r[k].reshape(sh))
            acc['R'].append(R)
            acc['t'].append(t)
        out = {k: np.stack(v) for k, v in acc.items()}
        out['K'], out['baseline'] = np.ascontiguousarray(s.K, dtype=np.float32), float(s.baseline)
        _BASE[shape] = out
    return _BASE[shape]


def punch(disp):
    """a block of zeros plus NaN, inf and negative entries: all of them invalid"""
    H, W = disp.shape[-2:]
    disp[..., H // 4:H // 4 + H // 6, W // 3:W // 3 + W // 5] = 0.0
    disp[..., H // 2, W // 2] = np.nan
    disp[..., H // 2 + 3, W // 4] = np.inf
    disp[..., (3 * H) // 4, (2 * W) // 3:(2 * W) // 3 + 2] = -1.5
    disp[..., 2, 5] = -np.inf


def make_input(shape, kind):
    """-> dict: disp (n, tl, H, W) float32, K (3, 3) float32, baseline, the truth R (n, tl, 3, 3), t (n, tl, 3) float32, R_pair, t_pair
    (float64), and of the exact track flow (n, tl tl, 2, H, W), visible (n, tl tl, H, W) bool and ambient (n, tl, H, W)"""
    key = (shape, kind)
    if key not in _INPUT:
        b = _render(shape)
        disp = b['disp'].astype(np.float32)
        if kind == 'holes':
            punch(disp)
        elif kind == 'noise':
            hit = disp > 0
            disp = np.where(hit, disp + np.random.RandomState(5).normal(0, 0.1, size=disp.shape).astype(np.float32), disp)
        out = {'disp': np.ascontiguousarray(disp, dtype=np.float32), 'K': b['K'], 'baseline': b['baseline'],
               'R': np.ascontiguousarray(b['R'], dtype=np.float32), 't': np.ascontiguousarray(b['t'], dtype=np.float32),
               'flow': b['flow'], 'visible': b['visible_in'].astype(bool), 'ambient': np.ascontiguousarray(b['ambient'], dtype=np.float32)}
        out['R_pair'], out['t_pair'] = pair_truth(out['R'], out['t'])
        _INPUT[key] = out
    return _INPUT[key]


def refs(shape, kind):
    """(float32 restatement, float64 restatement) at the defaults: computed once per case and never changed"""
    key = (shape, kind)
    if key not in _REF:
        a = make_input(shape, kind)
        _REF[key] = tuple(DR.align_poses(a['disp'], a['K'], a['baseline'], min_corr=MIN_CORR, dtype=dt) for dt in (np.float32, np.float64))
    return _REF[key]


def flow_chain(shape):
    """the parent's chain on the exact track: Horn-Schunck flow of the ambient images (flow_ref.dense_flow) -> pose_ref.track_poses"""
    if shape not in _FLOW:
        from tests import flow_ref, pose_ref
        a = make_input(shape, 'exact')
        fl = flow_ref.dense_flow(a['ambient'])['flow'].astype(np.float32)
        _FLOW[shape] = (fl, pose_ref.track_poses(a['disp'], fl, a['K'], a['baseline']))
    return _FLOW[shape]


def rot_angle(Ra, Rb):
    """the angle of Ra Rb^T over the leading axes, in rad"""
    M = np.einsum('...ab,...cb->...ac', np.asarray(Ra, dtype=np.float64), np.asarray(Rb, dtype=np.float64))
    return np.arccos(np.clip((np.trace(M, axis1=-2, axis2=-1) - 1) / 2, -1, 1))

