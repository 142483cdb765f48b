"""tests/adam_ref.py on its own: the fp32 restatement of csrc/adam.hip stays within the counted rounding bounds of the float64
Adam step on every gradient class, step count, gradient multiplier and learning rate that tests/test_adam_exact_gpu.py uses
(so bit equality with it on the device implies a correct step), follows torch.optim.Adam, and two subtly wrong variants of it
break the bounds (so the bounds have teeth)."""
import math

import numpy as np
import pytest
import torch

from tests import adam_ref as A

f32 = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8
COUNT = 332
GRAD_SCALES = (1.0, 0.125, 1.0 / 3.0)


def _walk(cls, t0, gs, lr, kind, variant=None, seed=0, clip=False):
    """NSTEPS steps of step32 (or a variant of it) from step number t0; yields per step the worst |step32 - step64| / bound
    for (m, v, p), every step measured from the fp32 state the trajectory itself reached.  clip: the multiplier is
    grad_scale * (float)coefficient of adam_ref.clip_setting, as adam_hyper_kernel forms it"""
    p, m, v = A.start(kind, COUNT, seed), np.zeros(COUNT, f32), np.zeros(COUNT, f32)
    for k, g in enumerate(A.gradients(cls, COUNT, seed)):
        t = t0 + k
        mult = f32(gs) * f32(A.clip_setting(g, gs)[2]) if clip else f32(gs)
        bc1, bc2s = A.host_bias_corrections(B1, B2, t)
        args = (p, g, m, v, lr, B1, B2, EPS)
        ref = A.step64(*args, t, mult)
        bnd = A.bounds(*args, t, mult)
        new = (variant or A.step32)(*args, bc1, bc2s, mult)
        worst = []
        for got, want, b in zip((new[1], new[2], new[0]), (ref[1], ref[2], ref[0]), bnd):
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(np.isfinite(err))
            worst.append(float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300)))))
        yield worst
        p, m, v = A.step32(*args, bc1, bc2s, mult)     # (variants are measured one step at a time, from correct states)


@pytest.mark.parametrize('cls', A.CLASSES)
def test_step32_is_within_the_counted_bounds_of_step64(cls):
    top = [0.0, 0.0, 0.0]
    for t0 in A.STEPS:
        for gs in GRAD_SCALES:
            for clip in (False, True):
                for lr in (1e-3, 1e-4):
                    for kind in ('zero', 'randn'):
                        for w in _walk(cls, t0, gs, lr, kind, seed=t0 % 97, clip=clip):
                            top = [max(a, b) for a, b in zip(top, w)]
    print(cls, 'worst error / bound: m %.3f v %.3f p %.3f' % tuple(top))
    assert max(top) <= 1.0, top


def test_counts_are_what_the_docstring_derives():
    assert (A.K_M, A.K_V, A.K_P) == (3, 4, 12) and A.U == 2.0 ** -24 and A.TINY == 2.0 ** -150
    z = np.zeros(4, f32)
    one = np.ones(4, f32)
    # |m| = |g| = 1: scale_m = 1, v' = 1 - b2 ... the bounds are K * (u * scale + TINY), one more rounding with a multiplier
    bm, bv, _ = A.bounds(z, one, one, z, 1e-3, B1, B2, EPS, 1, 1.0)
    assert np.allclose(bm, 3 * (A.U * 1.0 + A.TINY), rtol=1e-12) and np.allclose(bv, 4 * (A.U * (1 - B2) + A.TINY), rtol=1e-12)
    bm, bv, _ = A.bounds(z, one, one, z, 1e-3, B1, B2, EPS, 1, 0.5)
    assert np.allclose(bm, 4 * (A.U * 0.95 + A.TINY), rtol=1e-12) and np.allclose(bv, 6 * (A.U * 0.25 * (1 - B2) + A.TINY), rtol=1e-12)


def test_step32_trajectory_follows_torch_adam():
    """the project's bar for its optimiser: 5e-7 absolute on parameters of magnitude 1 (tests/test_adam_hyper_gpu.py)"""
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(COUNT, generator=g)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    p, m, v = p0.numpy().copy(), np.zeros(COUNT, f32), np.zeros(COUNT, f32)
    for t in range(1, 7):
        gr = torch.randn(COUNT, generator=g) * 10 ** (-(t - 1))
        pr.grad = gr.clone()
        opt.step()
        p, m, v = A.step32(p, gr.numpy(), m, v, 1e-3, B1, B2, EPS, *A.host_bias_corrections(B1, B2, t))
        d = float(np.abs(p - pr.detach().numpy()).max())
        print(t, 'max |step32 - torch| =', d)
        assert d < 5e-7
    st = opt.state[pr]
    assert float(np.abs(m - st['exp_avg'].numpy()).max()) < 5e-7 and float(np.abs(v - st['exp_avg_sq'].numpy()).max()) < 5e-7


# ------------------------------------------------------------------------------------------------ negative controls
def _omb2_in_float(p, g, m, v, lr, b1, b2, eps, bc1, bc2s, mult):
    """1 - beta2 formed in fp32: off by 1.3e-5 relative (the slip csrc/adam.hip's comment warns of)"""
    return A.step32(p, g, m, v, lr, b1, b2, eps, bc1, bc2s, mult, omb2=f32(1) - f32(b2))


def _eps_under_the_root(p, g, m, v, lr, b1, b2, eps, bc1, bc2s, mult):
    gr, m, v = A.moments32(g, m, v, b1, b2, mult)
    den = np.sqrt(v + f32(eps)) / f32(bc2s)
    return A.param32(p, m, den, lr, bc1), m, v


def test_control_one_minus_beta2_in_float_breaks_the_bounds():
    wm, wv, wp = (max(c) for c in zip(*_walk('randn', 1, 1.0, 1e-3, 'zero', _omb2_in_float)))
    print('omb2 = 1.f - (float)beta2: worst error / bound: m %.3g v %.3g p %.3g' % (wm, wv, wp))
    assert wm <= 1.0          # the first moment does not see it
    assert wv > 1.0 and wp > 1.0
    assert abs(float(f32(1) - f32(B2)) / (1.0 - B2) - 1.0) > 1e-5


@pytest.mark.parametrize('cls', ['randn', 'eps'])
def test_control_eps_under_the_root_breaks_the_bounds(cls):
    wm, wv, wp = (max(c) for c in zip(*_walk(cls, 1, 1.0, 1e-3, 'zero', _eps_under_the_root)))
    print(cls, 'eps under the root: worst error / bound: m %.3g v %.3g p %.3g' % (wm, wv, wp))
    assert wm <= 1.0 and wv <= 1.0      # the moments are untouched
    assert wp > 1.0


def test_host_bias_corrections_are_the_rounded_doubles():
    for t in (1, 2, 10, 1000, 100000):
        bc1, bc2s = A.host_bias_corrections(B1, B2, t)
        assert bc1 == f32(1.0 - math.pow(B1, t)) and bc2s == f32(math.sqrt(1.0 - math.pow(B2, t)))
    assert A.host_bias_corrections(B1, B2, 1) == (f32(1.0 - B1), f32(math.sqrt(1.0 - B2)))
