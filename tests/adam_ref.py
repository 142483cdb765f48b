"""TEST INFRASTRUCTURE: two references for ONE Adam step from a given fp32 state, and the bound that ties them together.

  step32   csrc/adam.hip's inner loop in numpy float32, rounding for rounding (the style of tests/bitexact.py): the library is
           built with -ffp-contract=off, so every product, sum, square root and quotient is rounded to fp32 on its own, and
           IEEE leaves one result for each.  A correct kernel returns THESE BITS.
  step64   torch.optim.Adam's formula in float64 with the Python-double hyper-parameters: what the step is meant to compute.
  bounds   how far a correct fp32 evaluation may be from step64, per element, by counting roundings (below).

tests/test_adam_ref_cpu.py shows that step32 stays within `bounds` of step64 on every gradient class of the GPU test: that
is what makes bit equality with step32 on the device imply a correct step.  Single steps from the kernel's own previous state
and not trajectories, because `exp_avg` is a signed sum: a bound relative to its value is off by orders of magnitude on random
data, the per-step scales below are tight.

THE COUNT.  u = 2^-24 is the relative error of one rounding to nearest; a rounding whose result is subnormal errs by at most
TINY = 2^-150 (half the smallest subnormal) instead, so every rounding contributes at most u * |its term| + TINY.  The fp32
constants (b1f, omb1, b2f, omb2, lr, bc1, bc2_sqrt, eps) are roundings of the double values step64 uses and count as such.
First order in u throughout.

  m' = m*b1f + gr*omb1                       scale_m = |m|*b1 + |gr|*(1 - b1)
       b1f, the product: 2 on the first term; omb1, the product: 2 on the second; the sum: 1 on |m'| <= scale_m.   K_M = 3
  v' = v*b2f + (gr*gr)*omb2                  scale_v = v' itself (both terms are >= 0)
       b2f, the product: 2 on the first term; gr*gr, omb2, the product: 3 on the second; the sum: 1.   K_V = max(2, 3) + 1 = 4
  p' = p - (lr/bc1) * (m' / den),  den = sqrt(v')/bc2_sqrt + eps
                                             scale_p = |p'| + |p' - p| + (lr/bc1) * scale_m / den
       the final difference: 1 on |p'|.
       on the update |p' - p|: lr, bc1, their quotient: 3; the quotient m'/den: 1; the product: 1; den: v' carries 4, halved
       by the root: 2, the root: 1, bc2_sqrt: 1, the quotient: 1, eps: 1, the sum: 1, together 7 (eps counted on top of the
       other term, not instead of it).  3 + 1 + 1 + 7 = 12.
       the error of m' (K_M * u * scale_m) reaches p' through (lr/bc1)/den: 3 on the third part of the scale.
       One K for the whole scale: K_P = max(1, 12, 3) = 12.
  mult != 1: gr = g*mult is one more rounding: +1 on the second term of m', +2 on gr*gr, hence +1 on den.   K + (1, 2, 1)

Underflow: K * TINY is added to each bound.  v' reaches p' through a square root, and |sqrt(a) - sqrt(b)| <= sqrt(|a - b|), so
the K_V * TINY of v' moves den by at most sqrt(K_V * TINY) / bc2_sqrt and p' by that share of the update; the K_M * TINY of m'
moves p' by (lr/bc1) * K_M * TINY / den.  (Both are below 1e-12 of the update with eps = 1e-8; they are written out because a
squared gradient that underflows to zero is one of the classes.)

Only tests/ may import this module."""
import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -150
K_M, K_V, K_P = 3, 4, 12


def _f(a):
    return np.asarray(a, f32)


def constants32(b1, b2):
    """b1f, omb1, b2f, omb2 as the entry points pass them: (float)beta and (float)(1.0 - beta), the difference in double"""
    return f32(b1), f32(1.0 - b1), f32(b2), f32(1.0 - b2)


def host_bias_corrections(b1, b2, t):
    """bc1, bc2_sqrt as dis_adam_step forms them on the host: double arithmetic, rounded once"""
    return f32(1.0 - b1 ** t), f32(math.sqrt(1.0 - b2 ** t))


def moments32(g, m, v, b1, b2, mult, omb1=None, omb2=None):
    """gr, m', v' of one step in fp32 (omb1 / omb2: other values for 1 - beta, for negative controls)"""
    b1f, d1, b2f, d2 = constants32(b1, b2)
    omb1 = d1 if omb1 is None else f32(omb1)
    omb2 = d2 if omb2 is None else f32(omb2)
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        gr = _f(g) * f32(mult)
        m = _f(m) * b1f + gr * omb1
        v = _f(v) * b2f + (gr * gr) * omb2
    return gr, m, v


def param32(p, m, den, lr, bc1):
    step = f32(lr) / f32(bc1)
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        return _f(p) - step * (_f(m) / _f(den))


def step32(p, g, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, mult=1.0, omb1=None, omb2=None):
    """-> (p', m', v'), float32 arrays: adam_kernel / adam_dev_kernel / adam_hyper_kernel term for term"""
    gr, m, v = moments32(g, m, v, b1, b2, mult, omb1, omb2)
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        den = np.sqrt(v) / f32(bc2_sqrt) + f32(eps)
    p = param32(p, m, den, lr, bc1)
    assert p.dtype == m.dtype == v.dtype == f32
    return p, m, v


def step64(p, g, m, v, lr, b1, b2, eps, t, mult=1.0):
    """-> (p', m', v') of step number t (1-based) in float64, torch.optim.Adam's single-tensor formula: the fp32 state and
    gradient taken as they are, `mult` the fp32 multiplier the kernel is given, everything else a Python double"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gr = g * float(f32(mult))
    m = m + (gr - m) * (1.0 - b1)                      # exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + gr * gr * (1.0 - b2)                  # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    den = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / den), m, v


def scales(p, g, m, v, lr, b1, b2, eps, t, mult=1.0):
    """-> (scale_m, scale_v, scale_p, update, den) of the module docstring, float64"""
    p64, m64, v64 = step64(p, g, m, v, lr, b1, b2, eps, t, mult)
    gr = np.abs(np.asarray(g, np.float64) * float(f32(mult)))
    sm = np.abs(np.asarray(m, np.float64)) * b1 + gr * (1.0 - b1)
    den = np.sqrt(v64) / math.sqrt(1.0 - b2 ** t) + eps
    upd = np.abs(p64 - np.asarray(p, np.float64))
    sp = np.abs(p64) + upd + (lr / (1.0 - b1 ** t)) * sm / den
    return sm, v64, sp, upd, den


def bounds(p, g, m, v, lr, b1, b2, eps, t, mult=1.0):
    """-> (bound_m, bound_v, bound_p): the largest |fp32 result - step64| a correct kernel may show, per element"""
    extra = (0, 0, 0) if float(f32(mult)) == 1.0 else (1, 2, 1)
    km, kv, kp = K_M + extra[0], K_V + extra[1], K_P + extra[2]
    sm, sv, sp, upd, den = scales(p, g, m, v, lr, b1, b2, eps, t, mult)
    step = lr / (1.0 - b1 ** t)
    bm = km * (U * sm + TINY)
    bv = kv * (U * sv + TINY)
    bp = kp * (U * sp + TINY) + upd * (math.sqrt(kv * TINY) / math.sqrt(1.0 - b2 ** t)) / den + step * km * TINY / den
    return bm, bv, bp


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
CLASSES = ('randn', 'eps', '1e-18', 'subnormal_sq', 'huge', 'mixed', 'sparse', 'decay')
STEPS = (1, 2, 10, 1000, 100000)
NSTEPS = 4


def gradients(cls, count, seed):
    """NSTEPS fresh fp32 gradients of one class, seeded:
    randn; eps: randn * 1e-8 (sqrt(v) comparable to eps); 1e-18; subnormal_sq: randn * 1e-21 (g * g subnormal or zero);
    huge: randn * 1e15; mixed: randn * 10^randint(-12, 6) per element; sparse: 70 % exact zeros; decay: two randn steps, then
    all-zero gradients (the moments decay, the parameter still moves)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(NSTEPS):
        r = rng.standard_normal(count)
        if cls == 'randn':
            g = r
        elif cls == 'eps':
            g = r * 1e-8
        elif cls == '1e-18':
            g = r * 1e-18
        elif cls == 'subnormal_sq':
            g = r * 1e-21
        elif cls == 'huge':
            g = r * 1e15
        elif cls == 'mixed':
            g = r * 10.0 ** rng.integers(-12, 7, count)
        elif cls == 'sparse':
            g = np.where(rng.random(count) < 0.7, 0.0, r)
        elif cls == 'decay':
            g = r if k < 2 else np.zeros(count)
        else:
            raise ValueError(cls)
        out.append(g.astype(f32))
    return out


def clip_setting(g, grad_scale):
    """-> (norm, max_norm, coefficient) of a clipped step as the GPU test sets it up: the float64 norm of the fp32 products
    g * grad_scale (what adam_norm_partials_kernel squares), an fp32 max_norm BELOW it (0.37 of it; 1 for a zero gradient), and
    torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) in float64"""
    s = (np.asarray(g, f32) * f32(grad_scale)).astype(np.float64)
    norm = math.sqrt(float(np.sum(s * s)))
    max_norm = float(f32(0.37 * norm)) if 0.0 < norm < math.inf else 1.0
    return norm, max_norm, min(1.0, max_norm / (norm + 1e-6))


def start(kind, count, seed):
    """starting parameters: 'zero' (the parameter IS the update) or 'randn'"""
    if kind == 'zero':
        return np.zeros(count, f32)
    return np.random.default_rng(seed + 7919).standard_normal(count).astype(f32)
