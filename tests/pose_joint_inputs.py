"""Inputs and cached restatements shared by the tests of the joint pose refinement (tests/test_pose_joint_ref_cpu.py,
tests/test_pose_joint_gpu.py, tests/test_pose_joint_pipeline_gpu.py): the inputs, shapes and parameters of tests/pose_inputs.py, the
kind `broken` on top of them, and the two starting points."""
import numpy as np

from tests import pose_inputs as PI
from tests import pose_joint_ref, pose_ref

SHAPES, PARAMS, MIN_CORR = PI.SHAPES, PI.PARAMS, PI.MIN_CORR
BROKEN_BASES = ['plane', 'noise', 'contam', 'render', 'holes']
KINDS = PI.INPUTS + [f'{k}+broken' for k in BROKEN_BASES]
BROKEN_PAIRS = ((0, 2), (2, 0))

_INPUT, _PAIRWISE, _INIT, _REF = {}, {}, {}, {}


def base_kind(kind):
    return kind.split('+')[0]


def has(shape, kind):
    """broken: at 64 x 96 and 130 x 70 only.  It needs a frame 2, and at 24 x 40 flow noise of 4 pixels is a tenth of the image: the
    pairwise start is then 0.5 rad off and the two restatements drift 1e-3 apart on the way back - the toy shape's geometry, as for
    contam in pose_inputs.has"""
    return PI.has(shape, base_kind(kind)) and (kind == base_kind(kind) or shape in (SHAPES[3], SHAPES[4]))


CASES = [(s, k) for s in SHAPES for k in KINDS if has(s, k)]


def case_id(c):
    return f'{PI.shape_id(c[0])}-{c[1]}'


def break_flows(flow, tl):
    """normal(0, 4) noise on the flows of the pairs (0, 2) and then (2, 0), from one generator: both pairs still fit (status 1), to
    a wrong pose"""
    flow = flow.copy()
    rng = np.random.RandomState(3)
    for (i, j) in BROKEN_PAIRS:
        flow[:, i * tl + j] += rng.normal(0, 4, size=flow[:, i * tl + j].shape).astype(np.float32)
    return flow


def make_input(shape, kind):
    """pose_inputs.make_input, with the broken flows where the kind asks for them (the base input is left unchanged)"""
    key = (shape, kind)
    if key not in _INPUT:
        a = PI.make_input(shape, base_kind(kind))
        if kind != base_kind(kind):
            a = dict(a, flow=break_flows(a['flow'], shape[1]))
        _INPUT[key] = a
    return _INPUT[key]


def pairwise(shape, kind):
    """the float64 pairwise restatement at PARAMS[0]"""
    key = (shape, kind)
    if key not in _PAIRWISE:
        if kind == base_kind(kind):
            _PAIRWISE[key] = PI.refs(shape, kind, 0)[1]
        else:
            a = make_input(shape, kind)
            _PAIRWISE[key] = pose_ref.track_poses(a['disp'], a['flow'], a['K'], a['baseline'], *PARAMS[0], MIN_CORR, dtype=np.float64)
    return _PAIRWISE[key]


def init(shape, kind, which='pairwise'):
    """the starting point, a fixed input computed once -> R (n, tl, 3, 3), t (n, tl, 3) float32, use (n, tl, tl) uint8 (the pairwise status).
    'pairwise': the float64 pairwise restatement, chained from frame 0 and rounded to float32 (the identity for a track no chain
    reaches); 'perturbed': the truth, every frame but frame 0 turned by 0.02 rad and shifted by 0.02"""
    key = (shape, kind, which)
    if key not in _INIT:
        from depthinspace_amd import synth
        from depthinspace_amd.data import presave_pose as PP
        n, tl = shape[:2]
        a, pw = make_input(shape, kind), pairwise(shape, kind)
        use = (pw['stats'][..., 3] != 0).astype(np.uint8)
        R = np.broadcast_to(np.eye(3, dtype=np.float32), (n, tl, 3, 3)).copy()
        t = np.zeros((n, tl, 3), np.float32)
        if which == 'pairwise':
            for b in range(n):
                got = PP.chain_track(pw['R_pair'][b], pw['t_pair'][b], use[b] != 0)
                if got is not None:
                    R[b], t[b] = got
        else:
            dR = synth._rodrigues(0.02 * np.array([2.0, -1.0, 2.0]) / 3.0)
            dt_ = 0.02 * np.array([1.0, 2.0, -2.0]) / 3.0
            for b in range(n):
                R[b, 0], t[b, 0] = a['R'][b, 0], a['t'][b, 0]
                for f in range(1, tl):
                    R[b, f] = dR @ a['R'][b, f].astype(np.float64)
                    t[b, f] = dR @ a['t'][b, f].astype(np.float64) + dt_
        _INIT[key] = (R, t, use)
    return _INIT[key]


def refs(shape, kind, pi, which='pairwise', masked=False):
    """(float32 restatement, float64 restatement) of the refinement: computed once per case and never changed.  masked: pair_use is
    the pairwise status (else NULL: every pair)"""
    key = (shape, kind, pi, which, masked)
    if key not in _REF:
        a = make_input(shape, kind)
        R, t, use = init(shape, kind, which)
        iters, scale, damping = PARAMS[pi]
        _REF[key] = tuple(pose_joint_ref.refine_track_poses(a['disp'], a['flow'], a['K'], a['baseline'], R, t, use if masked else None, iters,
                                                            scale, damping, MIN_CORR, dtype=dt) for dt in (np.float32, np.float64))
    return _REF[key]


def pose_error(R, t, a):
    """max |R_pair - truth| and max |t_pair - truth| over all pairs of the poses R (n, tl, 3, 3), t (n, tl, 3) against the truth of a"""
    Rp, tp = PI.pair_truth(R, t)
    return float(np.abs(Rp - a['R_pair']).max()), float(np.abs(tp - a['t_pair']).max())
