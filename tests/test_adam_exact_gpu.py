"""The three Adam entry points (csrc/adam.hip: dis_adam_step, dis_adam_step_dev, dis_adam_step_hyper in modes 0 - 3) against
tests/adam_ref.py, ONE STEP AT A TIME from the kernel's own previous fp32 state:

  * exp_avg, exp_avg_sq and the parameter equal adam_ref.step32 BIT FOR BIT (compared as 32-bit patterns: signed zeros and
    subnormal results included).  The library is built with -ffp-contract=off and every operation of the update is a correctly
    rounded IEEE one, so there is one right answer; tests/test_adam_ref_cpu.py shows that this answer is within the counted
    rounding bounds of the float64 step, so equality here means a correct step - an update wrong by 1e-5 of itself fails.
  * the parameter and both moments are within adam_ref.bounds of adam_ref.step64 (stands on its own feet).
  * the device step counter and bias corrections; the norm, the clip coefficient and the skip decision of the hyper form;
    elements past `count` and a guard region behind every buffer are untouched.

Gradient classes, step counts, multipliers and learning rates: adam_ref.CLASSES / STEPS, grad_scale in {1, 1/8, 1/3}, lr in
{1e-3, 1e-4}; parameters start at zero (the parameter is the update) or at randn.  Counts: 4, 332, the three-workgroup count
of tests/test_adam_hyper_gpu.py and 2048 * 256 * 4 + 4 * 77, the smallest ragged count that gives the update kernels a second
trip of their grid-stride loop (dis_ew_grid caps the grid at 2048 workgroups) and the norm 257 partials, one more than a
workgroup of adam_hyper_advance_kernel takes in one trip.

On an MI355X every class holds bit for bit, the parameter included: the device's sqrtf and division are correctly rounded on
these inputs, subnormal ones among them, so the parameter equality is not narrowed for any class.

The norm of the hyper form is compared with the float64 norm of the fp32 products g * grad_scale: those are the numbers the
kernel squares, and with grad_scale = 1/3 the exact products differ from them by 6e-8 relative, far above the 1e-10 bar."""
import math

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests.test_adam_hyper_gpu import _counts

pytestmark = pytest.mark.gpu

f32 = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8
GUARD = 64
SENTINEL = -7.25
ENTRIES = ('step', 'dev', 'hyper0', 'hyper1', 'hyper2', 'hyper3')
GRAD_SCALES = (1.0, 0.125, 1.0 / 3.0)
LRS = (1e-3, 1e-4)
COUNT_2M = 2048 * 256 * 4 + 4 * 77


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _ulps(a, b):
    """distance in representable floats (the bit patterns mapped to a monotonic integer line)"""
    def line(x):
        i = _bits(x).astype(np.int64)
        return np.where(i < 0x80000000, i, 0x80000000 - i)
    return np.abs(line(a) - line(b))


def _assert_same_bits(got, want, what):
    if not np.array_equal(_bits(got), _bits(want)):
        d = _ulps(got, want)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        i = int(bad[np.argmax(d[bad])])
        raise AssertionError(f'{what}: {bad.size} of {got.size} elements differ, worst {int(d[i])} ulp at [{i}]: '
                             f'{float(got[i])!r} != {float(want[i])!r}')


class _Case(object):
    """device buffers of one optimiser (count floats + GUARD sentinels each) and one checked step"""

    def __init__(self, entry, count, kind, t0, lr, gs, seed):
        from depthinspace_amd import lib
        self.entry, self.count, self.lr, self.gs, self.t = entry, count, lr, gs, t0 - 1
        self.mode = int(entry[5:]) if entry.startswith('hyper') else None
        self.tag = (entry, count, kind, t0, lr, gs)
        self.buf = {k: torch.full((count + GUARD,), SENTINEL, device='cuda') for k in 'pgmv'}
        self.host = {'p': A.start(kind, count, seed), 'm': np.zeros(count, f32), 'v': np.zeros(count, f32)}
        for k, a in self.host.items():
            self.buf[k][:count].copy_(torch.from_numpy(a))
        self.state = torch.tensor([t0 - 1, 0, 0, 0], dtype=torch.int32).cuda()
        self.hyper = torch.tensor([lr, 0.0, 0.0, 0.0], dtype=torch.float32).cuda()
        self.stats = torch.zeros(4, dtype=torch.float64).cuda()
        self.nparts = lib.fn('dis_adam_step_hyper_workspace')(count)
        self.partials = torch.full((self.nparts + 8,), SENTINEL, dtype=torch.float64, device='cuda')
        self.skipped = 0.0

    def _launch(self):
        from depthinspace_amd import ops
        n = self.count
        p, g, m, v = (self.buf[k][:n] for k in 'pgmv')
        kw = dict(beta1=B1, beta2=B2, eps=EPS, grad_scale=self.gs)
        if self.entry == 'step':
            ops.adam_step(p, g, m, v, self.t + 1, lr=self.lr, **kw)
        elif self.entry == 'dev':
            ops.adam_step_dev(p, g, m, v, self.state, lr=self.lr, **kw)
        elif self.mode == 0:
            ops.adam_step_hyper(p, g, m, v, self.state, self.hyper, **kw)
        else:
            ops.adam_step_hyper(p, g, m, v, self.state, self.hyper, self.stats, self.partials[:self.nparts], self.mode, **kw)
        torch.cuda.synchronize()

    def _read(self):
        n = self.count
        full = {k: self.buf[k].cpu().numpy() for k in 'pgmv'}
        for k, a in full.items():       # the guard region, and with it everything past `count`
            assert np.array_equal(_bits(a[n:]), _bits(np.full(GUARD, SENTINEL, f32))), (self.tag, 'guard of ' + k)
        assert np.array_equal(self.partials[self.nparts:].cpu().numpy(), np.full(8, SENTINEL)), (self.tag, 'guard of partials')
        return {k: a[:n] for k, a in full.items()}

    def step(self, g, inf_at=None):
        """one call on the fp32 gradient `g`, checked.  inf_at: index that is overwritten with +inf (the step must be skipped)"""
        n, tag = self.count, self.tag + (self.t + 1,)
        g = np.array(g, f32)
        if inf_at is not None:
            g[inf_at] = np.inf
        with np.errstate(over='ignore', invalid='ignore'):
            norm_ref, max_norm, _ = A.clip_setting(g, self.gs)    # (a max_norm below the norm: the coefficient is applied)
        clipping = self.mode is not None and self.mode & 1
        if clipping:
            self.hyper[1] = max_norm
        self.buf['g'][:n].copy_(torch.from_numpy(g))
        state_before = self.state.cpu().numpy().copy()
        self._launch()
        got = self._read()
        state = self.state.cpu().numpy()
        stats = self.stats.cpu().numpy()
        _assert_same_bits(got['g'], g, (tag, 'the gradient is an input'))

        mult = f32(self.gs)
        if self.mode:
            if math.isinf(norm_ref):
                assert stats[0] == math.inf, tag
            else:
                assert abs(stats[0] - norm_ref) <= 1e-10 * norm_ref, (tag, stats[0], norm_ref)
            if clipping:
                want = min(1.0, float(np.float64(f32(max_norm)) / (np.float64(stats[0]) + np.float64(1e-6))))
                assert stats[1] == want, (tag, stats[1], want)
                assert norm_ref == 0.0 or stats[1] < 1.0, tag
            else:
                assert stats[1] == 1.0, tag
            mult = f32(self.gs) * f32(stats[1])
            skip = bool(self.mode & 2) and inf_at is not None
            self.skipped += 1.0 if skip else 0.0
            assert stats[3] == (1.0 if skip else 0.0) and stats[2] == self.skipped, (tag, stats)
            if skip:
                for k in 'pmv':
                    _assert_same_bits(got[k], self.host[k], (tag, 'skipped step touched ' + k))
                assert np.array_equal(state, state_before), (tag, 'skipped step touched the state')
                return
        assert inf_at is None
        self.t += 1
        t = self.t
        hbc1, hbc2s = A.host_bias_corrections(B1, B2, t)
        if self.entry == 'step':
            assert np.array_equal(state, state_before)
            bc1, bc2s = hbc1, hbc2s
        else:
            assert int(state[0]) == t and int(state[3]) == 0, (tag, state)
            bc1, bc2s = state.view(f32)[1], state.view(f32)[2]
            # the device's pow is not correctly rounded, but the rounded float moves by one at the most
            assert _ulps(bc1, hbc1) <= 1 and _ulps(bc2s, hbc2s) <= 1, (tag, bc1, hbc1, bc2s, hbc2s)
            if t <= 10:
                assert bc1 == hbc1 and bc2s == hbc2s, (tag, bc1, hbc1, bc2s, hbc2s)
        prev = (self.host['p'], g, self.host['m'], self.host['v'], self.lr, B1, B2, EPS)
        p32, m32, v32 = A.step32(*prev, bc1, bc2s, mult)
        _assert_same_bits(got['m'], m32, (tag, 'exp_avg'))
        _assert_same_bits(got['v'], v32, (tag, 'exp_avg_sq'))
        _assert_same_bits(got['p'], p32, (tag, 'param'))
        p64, m64, v64 = A.step64(*prev, t, mult)
        for k, ref, b in zip('mvp', (m64, v64, p64), A.bounds(*prev, t, mult)):
            err = np.abs(got[k].astype(np.float64) - ref)
            assert np.all(err <= b), (tag, k, 'worst error / bound', float(np.max(err / np.maximum(b, 1e-300))))
        self.host = {k: got[k].copy() for k in 'pmv'}


def _pick(idx):
    return ('zero', 'randn')[idx % 2], GRAD_SCALES[idx % 3], LRS[(idx // 2) % 2]


@pytest.mark.parametrize('cls', A.CLASSES)
@pytest.mark.parametrize('entry', ENTRIES)
def test_every_class_at_every_step_count(entry, cls):
    """count 332 (329 real elements padded, ragged against a workgroup): every gradient class from every step count, NSTEPS
    fresh gradients each; start, grad_scale and learning rate cycle so that every value meets every class and entry point"""
    ei, ci = ENTRIES.index(entry), A.CLASSES.index(cls)
    for i, t0 in enumerate(A.STEPS):
        idx = ei * 7 + ci * len(A.STEPS) + i
        kind, gs, lr = _pick(idx)
        case = _Case(entry, 332, kind, t0, lr, gs, seed=idx)
        for g in A.gradients(cls, 332, seed=idx):
            case.step(g)
        assert case.t == t0 - 1 + A.NSTEPS


@pytest.mark.parametrize('cls', ['randn', 'mixed'])
@pytest.mark.parametrize('which', [0, 1, 2])
@pytest.mark.parametrize('entry', ENTRIES)
def test_every_count(entry, which, cls):
    """one float4, a ragged workgroup, three norm workgroups with a ragged last one"""
    count = _counts()[which]
    idx = ENTRIES.index(entry) * 5 + which * 3 + (cls == 'mixed')
    kind, gs, lr = _pick(idx)
    case = _Case(entry, count, kind, A.STEPS[idx % len(A.STEPS)], lr, gs, seed=100 + idx)
    for g in A.gradients(cls, count, seed=100 + idx):
        case.step(g)


@pytest.mark.parametrize('entry,cls,kind,t0,gs', [('step', 'mixed', 'zero', 1000, 1.0 / 3.0), ('dev', 'randn', 'randn', 1, 0.125),
                                                  ('hyper3', 'mixed', 'zero', 2, 1.0)])
def test_second_trip_of_the_grid_stride_loops(entry, cls, kind, t0, gs):
    """2,097,460 floats: 524,365 float4 against 2048 * 256 threads, 257 norm partials against a 256-thread reduction.  The hyper
    form (clip and skip on) then meets +inf in the last real element - the last, ragged partial: nothing moves, the skip is
    counted, and the next finite gradient is step t, not t + 1."""
    from depthinspace_amd import lib
    count = COUNT_2M
    assert count % 4 == 0 and count // 4 > 2048 * 256 and (count // 4 - 77) == 2048 * 256
    assert lib.fn('dis_adam_step_hyper_workspace')(count) == 257
    case = _Case(entry, count, kind, t0, 1e-3, gs, seed=7)
    grads = A.gradients(cls, count, seed=7)
    case.step(grads[0])
    case.step(grads[1])
    if entry == 'hyper3':
        case.step(grads[2], inf_at=count - 1)
        assert case.skipped == 1.0 and case.t == t0 + 1
    case.step(grads[2])
    assert case.t == t0 + 2


def test_skip_then_step_at_small_counts():
    """mode 2 alone (no clipping) and mode 3 at 332: +inf in element 0, then the same step number again"""
    for entry in ('hyper2', 'hyper3'):
        case = _Case(entry, 332, 'randn', 10, 1e-4, 0.125, seed=3)
        grads = A.gradients('randn', 332, seed=3)
        case.step(grads[0])
        case.step(grads[1], inf_at=0)
        case.step(grads[1], inf_at=331)
        case.step(grads[2])
        assert case.t == 11 and case.skipped == 2.0
