"""Plain statement of the GroupNorm(1 group) and activation kernels of csrc/norm_act.hip, torch on the CPU only, NHWC (n, hw, c).

Every function takes a `dtype`: float64 is the reference, float32 the fp32 yardstick - the same lines evaluated in fp32, reductions
by torch.sum.  The moments follow gn_moments (csrc/common.h): formed in fp64 from the sums, mean and rstd rounded to fp32, so the
fp64 reference shares the kernels' fp32 moments (raw=True: the unrounded fp64 moments, for the comparison with torch.autograd and
for the end-to-end test, where the sums are the kernel's own).

check() / check_sum() hold the two bars of tests/test_gn_fp64_gpu.py; there are no others.  Also here: the input generators, the
shape tables, and geometry() / chain_length(), which recompute grids, loop trip counts and the number of fp32 additions one
thread chains from the grid formulae of the entry points (dis_ew_grid, the caps 32 / 64 / 256 of dis_gn_stats, nred of
dis_gn_apply_bwd, slots x 256 of dis_gn_bwd_res_sums, ABB_BLOCKS)."""
import collections
import math

import torch

from depthinspace_amd.ops import ACT_NONE, ACT_SELU, ACT_RELU

F64, F32 = torch.float64, torch.float32
EPS = 1e-5
SELU_L = 1.0507009873554804934193349852946
SELU_A = 1.6732632423543772848170429916717
U32 = 2.0 ** -24
# common.h states the activations with float constants: SELU_SCALE_F and the product SELU_SCALE_F * SELU_ALPHA_F formed in fp32.  Like
# the moments they are shared with the reference (a stored y of exactly -lambda alpha has the derivative 0 on both sides);
# raw=True takes the exact constants instead
SELU_L32 = float(torch.tensor(SELU_L, dtype=torch.float32))
SELU_LA32 = float(torch.tensor(SELU_L, dtype=torch.float32) * torch.tensor(SELU_A, dtype=torch.float32))

# (a) of the elementwise bar: what test_group_norm (tests/test_net_ops_gpu.py) applies, of the largest |ref|; coefficients: y's
TOL = {'y': 2e-6, 'gpre': 2e-6, 'gx': 2e-5, 'gres': 1e-6, 'coef': 2e-6, 'gparam': 1e-5}
SUM_BAR = 1e-6       # reductions: |got - ref| <= SUM_BAR x sum |term|.  A thread chains at most MAX_CHAIN fp32 additions and a term
MAX_CHAIN = 8        # carries at most 3 roundings before everything continues in fp64: (8 + 3) 2^-24 = 6.6e-7
KINK = 1e-5          # end to end: gradient elements whose fp64 pre-activation lies this close to 0 are left out ...
EXCLUDE_CAP = 0.01   # ... at most this share of a case's elements


def dbl(t):
    return t.detach().to('cpu', F64)


# --------------------------------------------------------------------------------------------------
# the operations
# --------------------------------------------------------------------------------------------------
Moments = collections.namedtuple('Moments', 'mean rstd mean_raw rstd_raw var_raw')


def moments(stats, m, eps, dtype=F64):
    """gn_moments: mean = S1 / m, var = max(S2 / m - mean^2, 0), rstd = 1 / sqrt(var + eps) in fp64 (eps: the kernels' float),
    mean and rstd then rounded to fp32 and handed out in `dtype`; the raw fp64 values beside them"""
    st = dbl(stats).reshape(-1, 2)
    mu = st[:, 0] / m
    var = (st[:, 1] / m - mu * mu).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))
    return Moments(mu.to(F32).to(dtype), rs.to(F32).to(dtype), mu, rs, var)


def _mean_rstd(stats, m, eps, dtype, raw):
    mo = moments(stats, m, eps, dtype)
    if raw:
        return mo.mean_raw.to(dtype).view(-1, 1, 1), mo.rstd_raw.to(dtype).view(-1, 1, 1)
    return mo.mean.view(-1, 1, 1), mo.rstd.view(-1, 1, 1)


def stats(x, dtype=F64):
    """-> (n, 2) [sum x, sum x^2] per sample, and sum |x| (n) for the bars"""
    x = x.to(dtype)
    return torch.stack([x.sum(dim=(1, 2)), (x * x).sum(dim=(1, 2))], 1), x.abs().sum(dim=(1, 2))


def act_apply(v, act, raw=False):
    if act == ACT_SELU:
        lam, la = (SELU_L, SELU_L * SELU_A) if raw else (SELU_L32, SELU_LA32)
        return torch.where(v > 0, lam * v, la * (torch.exp(v) - 1.0))
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    return v


def act_grad_from_out(y, act, dtype=F64, raw=False):
    """the derivative of the activation through its OUTPUT (common.h): SELU: lambda when y > 0, else y + lambda alpha"""
    y = y.to(dtype)
    if act == ACT_SELU:
        lam, la = (SELU_L, SELU_L * SELU_A) if raw else (SELU_L32, SELU_LA32)
        return torch.where(y > 0, torch.full_like(y, lam), y + la)
    if act == ACT_RELU:
        return torch.where(y > 0, torch.ones_like(y), torch.zeros_like(y))
    return torch.ones_like(y)


def apply(x, st, gamma, beta, res, act, eps=EPS, dtype=F64, raw=False, pre=False):
    """act(x sc + sh (+ res)), sc = rstd gamma_c, sh = beta_c - sc mean (pre: the value in front of the activation)"""
    n, hw, c = x.shape
    mean, rstd = _mean_rstd(st, hw * c, eps, dtype, raw)
    sc = rstd * gamma.to(dtype)
    sh = beta.to(dtype) - sc * mean
    v = x.to(dtype) * sc + sh
    if res is not None:
        v = v + res.to(dtype)
    return v if pre else act_apply(v, act, raw)


def bwd(gy, y, x, st, gamma, act, in_act, eps=EPS, dtype=F64, raw=False):
    """the direct form: g = gy act'(y), gx = rstd (g gamma - a1 - xhat a2) (x act'(x) when in_act), gres = g,
    grad_gamma = sum g xhat, grad_beta = sum g; a1, a2 per sample; abs_gamma / abs_beta: the sums of the absolute terms"""
    n, hw, c = x.shape
    m = hw * c
    mean, rstd = _mean_rstd(st, m, eps, dtype, raw)
    g, xd, ga = gy.to(dtype), x.to(dtype), gamma.to(dtype)
    if act != ACT_NONE:
        g = g * act_grad_from_out(y, act, dtype, raw)
    xh = (xd - mean) * rstd
    t = g * ga
    a1 = t.sum(dim=(1, 2), keepdim=True) / m
    a2 = (t * xh).sum(dim=(1, 2), keepdim=True) / m
    gx = rstd * (t - a1 - xh * a2)
    if in_act != ACT_NONE:
        gx = gx * act_grad_from_out(xd, in_act, dtype, raw)
    gxh = g * xh
    return {'gx': gx, 'gres': g, 'grad_gamma': gxh.sum(dim=(0, 1)), 'grad_beta': g.sum(dim=(0, 1)), 'a1': a1.view(n), 'a2': a2.view(n),
            'abs_gamma': gxh.abs().sum(dim=(0, 1)), 'abs_beta': g.abs().sum(dim=(0, 1))}


def sums(g, x, dtype=F64):
    """A_c = sum_p g, B_c = sum_p g x per (sample, channel), and the sums of |g|, |g x|"""
    g, x = g.to(dtype), x.to(dtype)
    gx = g * x
    return g.sum(1), gx.sum(1), g.abs().sum(1), gx.abs().sum(1)


def coef(A, B, st, gamma, m, eps=EPS, dtype=F64, raw=False):
    """the comment above gn_coef_kernel: dbeta_c = A_c, dgamma_c = rstd (B_c - mean A_c), a1 = sum_c gamma_c A_c / M,
    a2 = sum_c gamma_c dgamma_c / M, k1_c = rstd gamma_c, kx = -rstd^2 a2, k0 = rstd^2 a2 mean - rstd a1"""
    mean, rstd = _mean_rstd(st, m, eps, dtype, raw)
    mean, rstd = mean.view(-1, 1), rstd.view(-1, 1)
    A, B, ga = A.to(dtype), B.to(dtype), gamma.to(dtype)
    dg = rstd * (B - mean * A)
    a1 = (ga * A).sum(1, keepdim=True) / m
    a2 = (ga * dg).sum(1, keepdim=True) / m
    kx = -(rstd * rstd) * a2
    k0 = (rstd * rstd) * a2 * mean - rstd * a1
    return {'k1': rstd * ga, 'kx': kx.view(-1), 'k0': k0.view(-1), 'grad_gamma': dg.sum(0), 'grad_beta': A.sum(0)}


def apply_coef(g, x, k1, kx, k0, in_act, dtype=F64):
    """gx = act'(x) (g k1_c + x kx + k0)"""
    n = x.shape[0]
    xd = x.to(dtype)
    gx = g.to(dtype) * k1.to(dtype).view(n, 1, -1) + (xd * kx.to(dtype).view(n, 1, 1) + k0.to(dtype).view(n, 1, 1))
    if in_act != ACT_NONE:
        gx = gx * act_grad_from_out(xd, in_act, dtype)
    return gx


# --------------------------------------------------------------------------------------------------
# the bars
# --------------------------------------------------------------------------------------------------
RECORD = []   # (family, output, case, kernel distance, yardstick distance [both in units of (a)], ratio): filled by the checks


def _maxerr(a, ref):
    e = (a - ref).abs()
    e = torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e)
    return float(e.max())


def check(got, ref, yard, tol, norm=None, sel=None, extra=0.0, family='', out='', case=''):
    """Elementwise outputs.  Error in the max norm over the set (`sel`: a region), normalised by the largest |ref| of the set
    (`norm`: another magnitude); bar = max((a) tol, (b) 4 x the fp32 yardstick's own distance to ref) + extra, where extra is the
    from-sums allowance of the elementwise pass from the coefficients.  The yardstick's distance never depends on `got`.
    -> error / bar; asserts that it is at most 1."""
    got, ref, yard = dbl(got), dbl(ref), dbl(yard)
    assert got.shape == ref.shape == yard.shape, (got.shape, ref.shape, yard.shape)
    if sel is not None:
        got, ref, yard = got[sel], ref[sel], yard[sel]
    assert ref.numel() > 0, (family, out, case)
    nrm = float(ref.abs().max()) if norm is None else float(norm)
    ek, ey = _maxerr(got, ref), _maxerr(yard, ref)
    if nrm == 0.0:   # an all-zero reference: only an exact zero passes
        dk, dy, ratio = (0.0 if ek == 0 else float('inf')), 0.0, (0.0 if ek == 0 else float('inf'))
    else:
        dk, dy = ek / nrm / tol, ey / nrm / tol
        ratio = (ek / nrm) / (max(tol, 4.0 * ey / nrm) + extra)
    RECORD.append((family, out, case, dk, dy, ratio))
    print(f'GNFP64 | {family} | {out} | {case} | kernel {dk:.3e} | yard {dy:.3e} | ratio {ratio:.3e}')
    assert ratio <= 1.0, (f'{family} {out} {case}: |kernel - fp64| is {ratio:.3e} x the bar max({tol:.1e}, 4 x yardstick) + {extra:.1e} of '
                          f'{nrm:.3e}; in units of {tol:.1e} the kernel is {dk:.3e} away, the yardstick {dy:.3e}')
    return ratio


def check_samples(got, ref, yard, tol, regions=(), extra=None, keep=None, family='', out='', case=''):
    """check() over all elements, per sample (each against its own largest |ref|) and per region [(name, mask)];
    extra: None or a function of the selection (None: everything, an int: that sample, a mask) -> allowance;
    keep: the elements that are compared at all (end to end: those away from a kink)"""
    ex = (lambda s: 0.0) if extra is None else extra
    worst = check(got, ref, yard, tol, sel=keep, extra=ex(None), family=family, out=out, case=case)
    if ref.dim() >= 1 and ref.shape[0] > 1:
        for s in range(ref.shape[0]):
            worst = max(worst, check(got[s], ref[s], yard[s], tol, sel=None if keep is None else keep[s], extra=ex(s), family=family,
                                     out=out, case=f'{case} [sample {s}]'))
    for name, mask in regions:
        mask = mask if keep is None else mask & keep
        if bool(mask.any()):
            worst = max(worst, check(got, ref, yard, tol, sel=mask, extra=ex(mask), family=family, out=out, case=f'{case} [{name}]'))
    return worst


def check_sum(got, ref, absterm, yard=None, family='', out='', case=''):
    """Reductions: |got - ref| <= SUM_BAR x sum |term| (absterm: the fp64 sum of the absolute values of what is summed), per
    element.  The yardstick takes no part in the bar; its distance is recorded for the table.  -> the largest error / bar"""
    got, ref, bar = dbl(got), dbl(ref), SUM_BAR * dbl(absterm)
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)

    def rel(a):
        e = (a - ref).abs()
        r = torch.where(e == 0, torch.zeros_like(e), e / bar)
        r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
        return float(r.max())
    ratio = rel(got)
    dy = rel(dbl(yard)) if yard is not None else float('nan')
    RECORD.append((family, out, case, ratio, dy, ratio))
    print(f'GNFP64 | {family} | {out} | {case} | kernel {ratio:.3e} | yard {dy:.3e} | ratio {ratio:.3e}')
    assert ratio <= 1.0, f'{family} {out} {case}: |kernel - fp64| is {ratio:.3e} x {SUM_BAR:.0e} x sum |term|'
    return ratio


# --------------------------------------------------------------------------------------------------
# shapes
# --------------------------------------------------------------------------------------------------
GN_MAXC = 128
SLOTS_FULL = 256     # dis_conv2d_gnsums_slots() on an MI355X: its compute units (the GPU tests ask the library)
SHAPES = collections.OrderedDict([
    ('one_vec', (1, 1, 4)),              # smallest legal: one float4, threads >= c idle
    ('one_round', (3, 256, 16)),         # exactly one round of one stats block
    ('one_past', (3, 257, 16)),          # one float4 row past it: second block, guarded tail
    ('odd_cg', (2, 143, 12)),            # c / 4 = 3: forward and stats only, the backward entry points refuse it
    ('maxc', (2, 37, 128)),              # c = GN_MAXC
    ('cap256', (1, 16512, 64)),          # stats: n < 4 cap, > 1 round; apply: 512-block cap, loop runs more than once
    ('cap64', (4, 8200, 32)),            # stats: cap 64, > 1 round; res_sums: more than one item per thread at all slots
    ('cap32', (16, 6200, 32)),           # stats: cap 32; reduce: nred 64, unrolled loop and tail; apply: 16 samples in reverse
    ('one_sample_big', (1, 16512, 128)),  # reduce: nred 512, unrolled loop; both apply kernels loop more than once
    ('old', (3, 143, 32)),               # the shape of test_group_norm: control
])
BWD_TAGS = [t for t, (n, hw, c) in SHAPES.items() if c % 4 == 0 and 256 % (c // 4) == 0]
SUMS_TAGS = [t for t, (n, hw, c) in SHAPES.items() if c in (4, 8, 16, 32)]
E2E_TAGS = ['old', 'cap32', 'one_past']


def res_sums_table(slots_full=SLOTS_FULL):
    """(tag, slots) of the dis_gn_bwd_res_sums tests: the full slot count on every from-sums shape, 1 and 8 slots where a thread
    then still chains at most MAX_CHAIN items (a block of 256 threads per slot walks the whole sample)"""
    rows = []
    for tag in SUMS_TAGS:
        for slots in (1, 8, slots_full):
            if slots == slots_full or chain_length('dis_gn_bwd_res_sums', *SHAPES[tag], slots) <= MAX_CHAIN:
                rows.append((tag, slots))
    return rows


COEF_SLOTS = (1, 16, 17, 240, 241, 256, 257, 511, 513)
COEF_C = (4, 16, 32)
COEF_N = (1, 3, 17)
COEF_HW = 1000

ACT_COUNTS = (4, 1024, 1028, 2049 * 256 * 4)
ACT_LD_C = (4, 16, 24, 32, 64)


def act_ld_npix(c):
    rows = 256 // (c // 4)
    return (1, rows - 1, rows, rows + 1, 1000, 1024 * rows + 3)


# --------------------------------------------------------------------------------------------------
# grids, trip counts, chains
# --------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def ew_grid(items, block=256):
    return max(1, min(2048, _cdiv(items, block)))


def geometry(kernel, n, hw, c, slots=None):
    """grid and loop trip counts of an entry point at a shape, from its host code's formulae; 'chain': fp32 additions one thread
    chains before the sum continues in fp64 (reduction kernels only)"""
    per4 = hw * (c // 4)
    if kernel == 'dis_gn_stats':
        cap = 32 if n >= 16 else (64 if n >= 4 else 256)
        gx = min(ew_grid(hw * c // 16), cap)
        span = 4 * gx * 256   # float4s of a sample that one round of its blocks covers
        # per round a thread adds 4 float4s in fp32: two tree levels inside a float4, then 4 accumulations
        return {'grid': gx, 'cap': cap, 'capped': ew_grid(hw * c // 16) > cap, 'rounds': _cdiv(per4, span), 'guarded_tail': per4 % span != 0,
                'chain': 6}
    if kernel in ('dis_gn_apply', 'dis_gn_bwd_apply_coef', 'dis_gn_bwd_from_sums'):
        gx = min(ew_grid(per4), 512)
        return {'grid': gx, 'capped': ew_grid(per4) > 512, 'trips': _cdiv(per4, gx * 256)}
    if kernel == 'dis_gn_apply_bwd':
        nred = _cdiv(512, n)
        nred = max(64, min(512, _cdiv(nred, 8) * 8))
        stride = nred * 256
        items = _cdiv(per4, stride)
        gxa = 2 * min(ew_grid(per4), 256)
        # (the body adds its 4 channels in fp32 before the fp64 sums; dgamma / dbeta chain one addition per item)
        return {'nred': nred, 'items': items, 'unrolled': per4 > 3 * stride, 'tail': per4 % (4 * stride) != 0, 'apply_grid': gxa,
                'apply_trips': _cdiv(per4, gxa * 256), 'chain': max(4, items)}
    if kernel == 'dis_gn_bwd_res_sums':
        items = _cdiv(per4, slots * 256)
        return {'items': items, 'chain': items}
    if kernel == 'dis_gn_bwd_coef':
        # thread (j, q) of a value takes the slots q, q + 16, ...: 16 per unrolled round (s + 240 < slots), the rest one by one; fp64
        rounds = tail = 0
        for q in range(16):
            s, r = q, 0
            while s + 240 < slots:
                s, r = s + 256, r + 1
            rounds, tail = max(rounds, r), max(tail, len(range(s, slots, 16)))
        return {'rounds': rounds, 'tail': tail, 'chain': 0}
    if kernel == 'dis_act_bwd_ld_bias':
        # (hw: the pixels).  A thread adds one value per pixel of its walk in fp32; rows, blocks and totals are added in fp64
        rows = 256 // (c // 4)
        nb = min(_cdiv(hw, rows), 1024)
        items = _cdiv(hw, nb * rows)
        return {'rows': rows, 'blocks': nb, 'items': items, 'chain': items}
    if kernel in ('dis_act_bwd', 'dis_add_act_fwd'):
        gx = ew_grid(hw // 4)
        return {'grid': gx, 'trips': _cdiv(hw // 4, gx * 256)}
    raise KeyError(kernel)


def chain_length(kernel, n, hw, c, slots=None):
    return geometry(kernel, n, hw, c, slots)['chain']


# --------------------------------------------------------------------------------------------------
# inputs (CPU generator: the same values on every machine with the same torch build)
# --------------------------------------------------------------------------------------------------
FWD_CASES = ('randn', 'offset30', 'offset1000', 'outlier_pixel', 'tiny_sample', 'constant_sample')
BWD_CASES = ('randn', 'offset30', 'outlier_pixel', 'tiny_sample', 'constant_sample', 'cancelling_g', 'selu_edges')
SUMS_CASES = ('randn', 'offset30', 'outlier_pixel', 'tiny_sample', 'cancelling_g', 'selu_edges')
ALL_CASES = ('randn', 'offset30', 'offset1000', 'outlier_pixel', 'tiny_sample', 'constant_sample', 'cancelling_g', 'selu_edges')
OFFSET_R = {'offset30': 30.0, 'offset1000': 1000.0}
CONST_VALUE = 5.1
ROW = 64   # cancelling_g: a sample's pixels in row blocks of 64; the patches lie in the first 16 pixels of a block


def _gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def selu_lambda_alpha_f32():
    return SELU_LA32


def selu_edges_(t, gen):
    """sets a few hundred entries of the SELU output t (in place) to exactly 0.0, -lambda alpha (fp32), the smallest positive
    subnormal and -0.0; -> their flat indices"""
    flat = t.view(-1)
    k = min(400, flat.numel() // 2)
    idx = torch.randperm(flat.numel(), generator=gen)[:k]
    vals = torch.tensor([0.0, -selu_lambda_alpha_f32(), 2.0 ** -149, -0.0], dtype=F32)
    flat[idx] = vals[torch.arange(k) % 4]
    return idx


def away_mask(n, hw, c):
    """cancelling_g: the elements away from the patches"""
    return ((torch.arange(hw) % ROW) >= 16).view(1, hw, 1).expand(n, hw, c)


def _patches(n, hw, c, gen):
    """a few O(1) 4 x 4 patches (4 row blocks x 4 pixels, all channels) in the first 16 pixels of the row blocks"""
    p = torch.zeros(n, hw, c, dtype=F64)
    nblk = _cdiv(hw, ROW)
    for s in range(n):
        for k in range(3):
            r0 = int(torch.randint(0, max(nblk - 3, 1), (1,), generator=gen))
            for r in range(r0, r0 + 4):
                lo, hi = min(r * ROW + 2 + 4 * k, hw), min(r * ROW + 6 + 4 * k, hw)
                if hi > lo:
                    p[s, lo:hi] = torch.randn(hi - lo, c, generator=gen).double()
    return p


_CACHE = {}


def inputs(case, tag):
    """-> dict of fp32 CPU tensors: x, gy, res (n, hw, c), gamma, beta (c), st (n, 2) the fp64 sums of x, y_edges (selu_edges:
    the stored SELU output).  Built once per (case, shape); the cache holds one shape at a time."""
    if _CACHE.get('tag') != tag:
        _CACHE.clear()
        _CACHE['tag'] = tag
    if case not in _CACHE:
        _CACHE[case] = _inputs(case, tag)
    return _CACHE[case]


def _inputs(case, tag):
    n, hw, c = SHAPES[tag]
    m = hw * c
    gen = _gen(ALL_CASES.index(case), list(SHAPES).index(tag))
    d = {'gamma': 1 + 0.2 * torch.randn(c, generator=gen), 'beta': 0.2 * torch.randn(c, generator=gen)}
    x = 1.5 * torch.randn(n, hw, c, generator=gen) + 0.3
    gy = torch.randn(n, hw, c, generator=gen)
    d['res'] = torch.randn(n, hw, c, generator=gen)
    if case in OFFSET_R:
        z = torch.randn(n, hw, c, generator=gen).double()   # standardised per sample: mean / std is R at every shape
        z = (z - z.mean(dim=(1, 2), keepdim=True)) / z.std(dim=(1, 2), keepdim=True, unbiased=False)
        x = (OFFSET_R[case] + z).float()
    elif case == 'outlier_pixel':
        x[0, hw // 2, :] = 1e4
        gy[1 % n, hw // 3, 3 % c] = 1e4
    elif case == 'tiny_sample':
        if n > 1:
            x[1] *= 1e-6
            gy[1] *= 1e-6
    elif case == 'constant_sample':
        x[0] = CONST_VALUE
    elif case == 'cancelling_g':
        # dL/dxhat = alpha + beta xhat away from the patches, which are made orthogonal to 1 and xhat: alpha and beta ARE the two
        # means of the backward, and gx cancels to the rounding of g there (spread 30: var >> eps, the xhat direction cancels too)
        x = 30.0 * torch.randn(n, hw, c, generator=gen)
        mo = moments(stats(x)[0], m, EPS)
        xh = (x.double() - mo.mean.view(n, 1, 1)) * mo.rstd.view(n, 1, 1)
        sgn = lambda: (torch.randint(0, 2, (n, 1, 1), generator=gen) * 2 - 1).double()
        al = sgn() * (0.5 + torch.rand(n, 1, 1, generator=gen).double()) * 4e3
        be = sgn() * (0.5 + torch.rand(n, 1, 1, generator=gen).double()) * 4e3
        p = _patches(n, hw, c, gen)
        on = (p != 0).double()
        for s in range(n):
            k = on[s].sum()
            if k < 3:
                p[s] = 0
                continue
            h1, h2 = (xh[s] * on[s]).sum(), (xh[s] * xh[s] * on[s]).sum()
            s1, s2 = p[s].sum(), (p[s] * xh[s]).sum()
            det = k * h2 - h1 * h1           # u k + v h1 = s1, u h1 + v h2 = s2
            u, v = (s1 * h2 - s2 * h1) / det, (k * s2 - h1 * s1) / det
            p[s] = p[s] - (u + v * xh[s]) * on[s]
        gy = ((al + be * xh + p) / d['gamma'].double()).float()
    elif case == 'selu_edges':
        x = torch.nn.functional.selu(1.5 * torch.randn(n, hw, c, generator=gen))
        selu_edges_(x, gen)
        d['y_edges'] = torch.nn.functional.selu(1.5 * torch.randn(n, hw, c, generator=gen))
        selu_edges_(d['y_edges'], gen)
    d['x'], d['gy'] = x.contiguous(), gy.contiguous()
    d['st'] = stats(d['x'])[0]
    return d


def stored_y(d, act, has_res):
    """the fp32 y a backward kernel is handed: the reference's own output of the forward pass rounded to fp32 (selu_edges: the
    prepared SELU output).  Both sides of a C-ABI backward comparison branch on these stored bits: no kinks."""
    if 'y_edges' in d:
        return d['y_edges']
    return apply(d['x'], d['st'], d['gamma'], d['beta'], d['res'] if has_res else None, act).float()


def act_ld_inputs(npix, c, act, seed):
    """gy and y as channel ranges [off, off + c) of wider buffers (ldg, ldy floats per pixel, every other column NaN: a read
    outside the range shows in the output); y in selu_edges form"""
    gen = _gen(npix, c, act, seed)
    ldg, ldy, offg, offy = c + 8, c + 12, 4, 8
    gbuf = torch.full((npix, ldg), float('nan'))
    ybuf = torch.full((npix, ldy), float('nan'))
    gy = torch.randn(npix, c, generator=gen)
    y = torch.nn.functional.selu(1.5 * torch.randn(npix, c, generator=gen))
    selu_edges_(y, gen)
    gbuf[:, offg:offg + c] = gy
    ybuf[:, offy:offy + c] = y
    return gbuf, ybuf, gy, y, (ldg, ldy, offg, offy)


ADD_ACT_SPECIALS = (0.0, 1e-30, -1e-30, -20.0, -90.0, 1e4)


def add_act_inputs(count, seed):
    """a, b with a + b on exact 0, +-tiny, -20, -90 and +1e4 at a few places (b = 0 there); -> a, b, mask of the 1e4 entries"""
    gen = _gen(count, seed)
    a, b = 2 * torch.randn(count, generator=gen), torch.randn(count, generator=gen)
    k = min(count // 2, 60)
    idx = torch.randperm(count, generator=gen)[:k]
    a[idx] = torch.tensor(ADD_ACT_SPECIALS, dtype=F32)[torch.arange(k) % len(ADD_ACT_SPECIALS)]
    b[idx] = 0.0
    return a, b, (a + b) == 1e4


def coef_inputs(slots, n, c, seed=0):
    """ab (n, slots, 2, c) doubles: every slot holds A / slots + noise of mixed magnitude, randn 10^U(-6, 0); stats of a sample
    with mean 0.3 and variance 2.25 over COEF_HW pixels"""
    gen = _gen(slots, n, c, seed)
    m = COEF_HW * c
    base = torch.randn(n, 1, 2, c, generator=gen, dtype=F64) * math.sqrt(COEF_HW)
    noise = torch.randn(n, slots, 2, c, generator=gen, dtype=F64) * 10.0 ** (-6.0 * torch.rand(n, slots, 2, c, generator=gen, dtype=F64))
    ab = (base / slots + noise).contiguous()
    mu = 0.3 + 0.05 * torch.randn(n, generator=gen, dtype=F64)
    st = torch.stack([mu * m, (2.25 + mu * mu) * m], 1).contiguous()
    gamma = 1 + 0.2 * torch.randn(c, generator=gen)
    return ab, st, gamma


def kink_keep(pre, act):
    """end to end: the gradient elements that are compared - those whose fp64 pre-activation is not within KINK of 0"""
    if act == ACT_NONE:
        return torch.ones_like(pre, dtype=torch.bool)
    return pre.abs() > KINK


def excluded_share(keep):
    return 1.0 - float(keep.to(F64).mean())
