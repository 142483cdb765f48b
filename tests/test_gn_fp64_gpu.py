"""The GroupNorm(1 group) and activation kernels of csrc/norm_act.hip, called through the C ABI (lib.call; the end-to-end test
through ops.group_norm), against the plain fp64 statements of tests/gn_ref.py - at shapes taken from the kernels' own constants
(gn_ref.SHAPES: the smallest legal tensor, exactly one round of one block, one float4 row past it, c / 4 = 3, c = GN_MAXC, each of
the three grid caps of dis_gn_stats with more than one round, the unrolled loop of the backward reduce with its tail, grid-stride
loops that run more than once; tests/test_gn_ref_cpu.py recomputes every claim from the grid formulae) and on inputs that a conv
output can reach: mean / deviation 30 and 1000, one 1e4 pixel, one sample at 1e-6, a constant sample (var = 0: eps decides), a
gradient that the backward cancels to its own rounding away from a few patches, and SELU outputs on the edges of act' (exactly
0.0, -0.0, -lambda alpha, the smallest subnormal).  The moments of the C-ABI tests come from the host in fp64 and the backward
kernels are handed y and x as stored fp32 values, so both sides branch on the same bits and every element is compared.

BARS (gn_ref.check / check_sum; there are no others in this file).
  Elementwise outputs (y, gx, gres, gpre, coefficients): max norm over all elements, per sample, and for cancelling_g over the
    region away from the patches, normalised by the largest |ref| of that set; bar = the larger of (a) the tolerance of
    test_group_norm (y, gpre 2e-6, gx 2e-5, gres 1e-6, coefficients 2e-6, parameter gradients end to end 1e-5) and (b) 4 x the fp32
    yardstick's own distance to fp64 on the same inputs (gn_ref's lines in fp32; never the kernel's output).  The elementwise pass
    from the coefficients alone gets 4 x 2^-24 max(|x kx|, |k0|) / max |ref| on top: the fp32 rounding of the cancelling pair
    x kx + k0, which the direct-form yardstick does not have.
  Reductions (S1, S2, A, B, grad_gamma, grad_beta, the bias gradient): |got - ref| <= 1e-6 sum |term|.  Derived: at these shapes a
    thread chains at most 8 fp32 additions (test_gn_ref_cpu.py holds that) and a term carries at most 3 roundings before everything
    continues in fp64: 11 x 2^-24 = 6.6e-7.  dis_gn_bwd_res_sums at 1 and 8 slots runs on the shapes where that still holds
    (gn_ref.res_sums_table).
  End to end the kernel branches on its own fp32 y: gradient elements whose fp64 pre-activation lies within 1e-5 of 0 are left out
    (at most 1 % of a case, asserted; about 1e-5 of it with these inputs), and the parameter gradients, which sum over those
    elements too, are allowed the sum of what the left-out elements could contribute on the other branch.

CHANGED WITH THIS FILE.  The bias gradient of dis_act_bwd_ld_bias added the rows of a block (256 / (c / 4): up to 256 of them) in
one fp32 chain behind the per-thread chain, where the reduction bar is derived for 8 additions.  The rows are now added in fp64
(norm_act.hip), gn_ref.chain_length('dis_act_bwd_ld_bias', ...) is 2 at the largest pixel count and the bar holds by derivation.
(On these random-sign inputs the fp32 chain stayed inside the bar as well: the change is for the worst case, not a measured miss.)

OBSERVED, not changed.  (1) dis_gn_stats squares in fp32: the variance that follows from its sums is up to 6.1e-5 (R = 30) and
6.3e-2 (R = 1000) of var away from fp64 at 4 elements, 2e-7 .. 9e-6 and 2e-4 .. 5e-3 at the larger shapes (rstd: half of that) -
inside 1e-6 S2 / m, which is 9e-4 and 1.0 of var.  (2) y = x sc + sh with sc = gamma rstd: on a constant sample (rstd = 316) y
is beta only to 1.2e-4 absolute (three roundings of |x sc| = 2e3; the fp32 yardstick is the same).  (3) Where a whole sample is
constant or cancels entirely (1 x 1 x 4 under outlier_pixel and cancelling_g) kernel and yardstick are the same 0.1 .. 0.3 of the
tiny result from fp64: the 1e5 golden tolerances in the table; (b) is the bar there.

MEASURED (MI355X).  `kernel`, `yard`: distance to fp64 in units of (a) for elementwise outputs (1 or less: (a) alone holds; above
1 the yardstick is as far, and (b) is the bar) and in units of 1e-6 sum |term| for reductions; the largest over the family's
comparisons (all / per sample / region each count as one).  `ratio`: |kernel - fp64| / bar, the largest - 1 would be the bar.
  family          output      checks    kernel      yard    ratio   comparison of the largest ratio
  gn_stats        S1              60   5.3e-02   2.2e-01    0.053   one_vec tiny_sample
  gn_stats        S2              60   4.0e-02   3.4e-01    0.040   one_sample_big outlier_pixel
  gn_apply        y             1032   1.4e+05   1.4e+05    0.255   one_past offset30 act1 res0   (1.4e5: one_vec outlier_pixel, see (3))
  gn_apply_bwd    gx            1152   1.5e+05   1.5e+05    0.565   old cancelling_g act0 res0 in1   (1.5e5: one_vec cancelling_g)
  gn_apply_bwd    gres           560   9.5e-02   9.5e-02    0.095   one_round randn act1 res1 in0 [sample 2]
  gn_apply_bwd    grad_gamma     252   1.2e-01   2.6e-01    0.118   maxc outlier_pixel act1 res1 in0
  gn_apply_bwd    grad_beta      252   5.4e-02   2.0e-01    0.054   maxc outlier_pixel act1 res1 in0
  gn_res_sums     A              294   1.2e-01   1.6e-01    0.125   old slots1 outlier_pixel act1
  gn_res_sums     B              294   1.1e-01   4.8e-01    0.115   old slots1 outlier_pixel act2
  gn_res_sums     gres           854   9.5e-02   9.5e-02    0.095   one_round slots1 randn act1 [sample 2]
  gn_coef         k1             621   2.7e-02   2.7e-02    0.027   slots511 c32 n17
  gn_coef         kx             621   5.8e-02   2.0e+01    0.058   slots513 c4 n3 [sample 2]
  gn_coef         k0             621   1.1e+00   1.1e+02    0.250   slots256 c16 n17 [sample 10]   (k0 cancels there; the yardstick is 100 x further)
  gn_coef         grad_gamma      81   5.8e-02   1.1e-01    0.058   slots1 c32 n1
  gn_coef         grad_beta       81   5.5e-02   9.3e-02    0.055   slots16 c32 n1
  gn_from_coef    gx             430   1.0e+05   1.5e+05    0.414   old cancelling_g in1
  gn_from_coef    grad_gamma      36   4.1e-02   1.4e-01    0.041   one_past outlier_pixel
  gn_from_coef    grad_beta       36   5.3e-02   1.2e-01    0.053   cap64 cancelling_g
  group_norm      y              150   1.6e+00   4.0e+01    0.791   old offset30 act0 res0 [sample 2]   (fp32 sums of x^2 at R = 30: the yardstick)
  group_norm      gx             150   2.8e-01   1.7e+04    0.276   old offset30 act1 res0 [sample 2]
  group_norm      gres            50   4.2e+00   3.5e+05    0.392   old offset30 act1 res1 [sample 2]
  group_norm      grad_gamma      18   2.8e+01   5.7e+02    0.164   cap32 offset30 act1 res0
  group_norm      grad_beta       18   7.9e+01   2.3e+02    0.146   cap32 offset30 act1 res0
  act_bwd         gpre            12   3.2e-02   3.2e-02    0.032   count 2098176 act1
  act_bwd_ld      gpre            90   3.7e-02   3.7e-02    0.037   c24 npix 1000 act1
  act_bwd_ld_bias bias_grad       72   7.8e-02   1.2e-01    0.078   c32 npix 1 act1
  add_act         y               21   3.8e-02   3.8e-02    0.038   count 2098176 act1 [without the 1e4 entries]
The largest share of elements left out end to end is 8.8e-6.  The whole file takes 14 s on an MI355X host (358 tests, none
above 0.8 s), most of it the CPU's fp64 and fp32 references.  Scratch builds with one line changed each fail it where they should:
dis_gn_stats dropping every round after the first (the 30 tests on the three cap shapes), the unrolled loop of the backward
reduce dropping its fourth load (20: cap32 and one_sample_big), the unrolled slot round of gn_coef_kernel dropping its last
slot (the 5 slot counts from 241 up), act' taking y >= 0 for y > 0 (177: every case that holds an exact 0).
"""
import pytest
import torch

from tests import gn_ref as G

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
GUARD, SENTINEL = 64, 12345.0
COMBOS_FWD = [(0, False), (1, True), (1, False), (2, True)]                       # (act, residual)
COMBOS_BWD = [(0, False, 0), (1, True, 0), (0, False, 1), (2, True, 0)]           # (act, residual gradient, in_act)
COMBOS_SUMS = [(1, True), (0, False), (2, True)]                                  # (act, gres stored)


def _lib():
    from depthinspace_amd import lib
    return lib


def _dev(d):
    """the case's tensors on the device, once per case"""
    if '_dev' not in d:
        d['_dev'] = {k: (v.cuda() if k != 'st' else v.reshape(-1).contiguous().cuda()) for k, v in d.items() if isinstance(v, torch.Tensor)}
    return d['_dev']


def _nan(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _regions(case, n, hw, c):
    return [('away from the patches', G.away_mask(n, hw, c))] if case == 'cancelling_g' else []


def _coef_buf(n, c):
    return _nan(n * (c + 2) + 4 * n * c + 2)


# ---------------------------------------------------------------------------------------------------------------- a. statistics
@pytest.mark.parametrize('case', G.FWD_CASES)
@pytest.mark.parametrize('tag', list(G.SHAPES))
def test_gn_stats(tag, case):
    """the sums are added atomically onto a zeroed pair, once; in the offset cases the variance and rstd that follow from the
    kernel's sums are printed against fp64 and the variance held to 1e-6 S2 / m (loose at R = 1000 by construction)"""
    lib = _lib()
    n, hw, c = G.SHAPES[tag]
    d = G.inputs(case, tag)
    st = torch.zeros(2 * n, dtype=F64, device='cuda')
    lib.call('dis_gn_stats', _dev(d)['x'], st, n, hw * c)
    got = st.view(n, 2).cpu()
    (ref, sabs), (yard, _) = G.stats(d['x']), G.stats(d['x'], F32)
    assert G.chain_length('dis_gn_stats', n, hw, c) <= G.MAX_CHAIN
    G.check_sum(got[:, 0], ref[:, 0], sabs, yard[:, 0], 'gn_stats', 'S1', f'{tag} {case}')
    G.check_sum(got[:, 1], ref[:, 1], ref[:, 1], yard[:, 1], 'gn_stats', 'S2', f'{tag} {case}')
    if case in G.OFFSET_R:
        m = hw * c
        mk, mr = G.moments(got, m, G.EPS), G.moments(ref, m, G.EPS)
        dvar = (mk.var_raw - mr.var_raw).abs()
        ev, er = float((dvar / mr.var_raw).max()), float(((mk.rstd_raw - mr.rstd_raw).abs() / mr.rstd_raw).max())
        print(f'GNVAR | {tag} {case} | var {ev:.3e} | rstd {er:.3e} | bound {float((1e-6 * ref[:, 1] / m / mr.var_raw).max()):.3e}')
        assert bool((dvar <= 1e-6 * ref[:, 1] / m).all()), (ev, er)


# ---------------------------------------------------------------------------------------------------------------- b. forward
@pytest.mark.parametrize('case', G.FWD_CASES)
@pytest.mark.parametrize('tag', list(G.SHAPES))
def test_gn_apply(tag, case):
    lib = _lib()
    n, hw, c = G.SHAPES[tag]
    d = G.inputs(case, tag)
    D = _dev(d)
    for act, res in COMBOS_FWD:
        y = _nan(n, hw, c)
        lib.call('dis_gn_apply', D['x'], D['st'], D['gamma'], D['beta'], D['res'] if res else None, y, n, hw, c, act, G.EPS)
        y = y.cpu()
        assert not bool(torch.isnan(y).any())
        r = d['res'] if res else None
        ref = G.apply(d['x'], d['st'], d['gamma'], d['beta'], r, act)
        yard = G.apply(d['x'], d['st'], d['gamma'], d['beta'], r, act, dtype=F32)
        G.check_samples(y, ref, yard, G.TOL['y'], family='gn_apply', out='y', case=f'{tag} {case} act{act} res{int(res)}')
        if case == 'constant_sample' and act == 0 and not res:
            # var = 0: xhat = 0 and y = beta, up to the three roundings of magnitude |x sc| in x sc + (beta - sc mean), sc = gamma / sqrt(eps)
            dev = float((y[0].double() - d['beta'].double()).abs().max())
            big = G.CONST_VALUE * float(G.moments(d['st'], hw * c, G.EPS).rstd[0]) * float(d['gamma'].abs().max())
            print(f'GNCONST | {tag} | max |y - beta| {dev:.3e} | 3 x 2^-24 |x sc| {3 * G.U32 * big:.3e}')
            assert dev <= 3 * G.U32 * big


# ---------------------------------------------------------------------------------------------------------------- c. two-pass backward
def _apply_bwd(lib, D, y, n, hw, c, act, has_res, in_act):
    wtot = lib.fn('dis_gn_bwd_workspace')(n, c)
    nred2 = wtot // (2 + 2 * c) * 2       # as ops._gn_apply_bwd splits it
    ws = _nan(wtot, dtype=F64)            # every slot that is read must have been written
    gx, gres, gg, gb = _nan(n, hw, c), (_nan(n, hw, c) if has_res else None), _nan(c), _nan(c)
    lib.call('dis_gn_apply_bwd', D['gy'], y, D['x'], D['st'], D['gamma'], gx, gres, gg, gb, ws[:nred2], ws[nred2:], n, hw, c, act, G.EPS,
             in_act)
    return [t.cpu() if t is not None else None for t in (gx, gres, gg, gb)]


@pytest.mark.parametrize('case', G.BWD_CASES)
@pytest.mark.parametrize('tag', G.BWD_TAGS)
def test_gn_apply_bwd(tag, case):
    lib = _lib()
    n, hw, c = G.SHAPES[tag]
    assert G.chain_length('dis_gn_apply_bwd', n, hw, c) <= G.MAX_CHAIN
    d = G.inputs(case, tag)
    D = _dev(d)
    for act, has_res, in_act in COMBOS_BWD:
        y = G.stored_y(d, act, has_res) if act else None
        yd = y.cuda() if act else None
        a = _apply_bwd(lib, D, yd, n, hw, c, act, has_res, in_act)
        b = _apply_bwd(lib, D, yd, n, hw, c, act, has_res, in_act)
        for u, v in zip(a, b):   # fixed summation orders: bit for bit on repeat
            assert u is None or torch.equal(u, v)
        gx, gres, gg, gb = a
        ref = G.bwd(d['gy'], y, d['x'], d['st'], d['gamma'], act, in_act)
        yard = G.bwd(d['gy'], y, d['x'], d['st'], d['gamma'], act, in_act, dtype=F32)
        what = f'{tag} {case} act{act} res{int(has_res)} in{in_act}'
        G.check_samples(gx, ref['gx'], yard['gx'], G.TOL['gx'], regions=_regions(case, n, hw, c), family='gn_apply_bwd', out='gx', case=what)
        if has_res:
            G.check_samples(gres, ref['gres'], yard['gres'], G.TOL['gres'], family='gn_apply_bwd', out='gres', case=what)
        G.check_sum(gg, ref['grad_gamma'], ref['abs_gamma'], yard['grad_gamma'], 'gn_apply_bwd', 'grad_gamma', what)
        G.check_sum(gb, ref['grad_beta'], ref['abs_beta'], yard['grad_beta'], 'gn_apply_bwd', 'grad_beta', what)


# ---------------------------------------------------------------------------------------------------------------- d. channel sums
@pytest.mark.parametrize('case', G.BWD_CASES)
@pytest.mark.parametrize('tag,slots', G.res_sums_table())
def test_gn_bwd_res_sums_fp64(tag, slots, case):
    lib = _lib()
    n, hw, c = G.SHAPES[tag]
    if slots == G.SLOTS_FULL:
        slots = int(lib.fn('dis_conv2d_gnsums_slots')())
    assert G.chain_length('dis_gn_bwd_res_sums', n, hw, c, slots) <= G.MAX_CHAIN
    d = G.inputs(case, tag)
    D = _dev(d)
    for act, store in COMBOS_SUMS:
        y = G.stored_y(d, act, True) if act else None
        yd = y.cuda() if act else None
        runs = []
        for _ in range(2):
            ab = _nan(n, slots, 2, c, dtype=F64)   # "every slot written"
            gres = _nan(n, hw, c) if store else None
            lib.call('dis_gn_bwd_res_sums', D['gy'], yd, D['x'], gres, ab, slots, n, hw, c, act)
            runs.append((ab.cpu(), gres.cpu() if store else None))
        assert torch.equal(runs[0][0], runs[1][0]) and (not store or torch.equal(runs[0][1], runs[1][1]))
        ab, gres = runs[0]
        assert not bool(torch.isnan(ab).any())
        g64 = d['gy'].double() * G.act_grad_from_out(y, act) if act else d['gy'].double()
        g32 = d['gy'] * G.act_grad_from_out(y, act, F32) if act else d['gy']
        A, B, absA, absB = G.sums(g64, d['x'])
        A32, B32, _, _ = G.sums(g32, d['x'], F32)
        what = f'{tag} slots{slots} {case} act{act}'
        got = ab.sum(dim=1)
        G.check_sum(got[:, 0], A, absA, A32, 'gn_res_sums', 'A', what)
        G.check_sum(got[:, 1], B, absB, B32, 'gn_res_sums', 'B', what)
        if store:
            G.check_samples(gres, g64, g32, G.TOL['gres'], family='gn_res_sums', out='gres', case=what)


# ---------------------------------------------------------------------------------------------------------------- e. slot summation
@pytest.mark.parametrize('slots', G.COEF_SLOTS)
def test_gn_coef_slot_summation(slots):
    """every slot filled (A / slots + noise of mixed magnitude); coefficients and parameter gradients of dis_gn_bwd_coef against the
    statement above gn_coef_kernel on the host's fp64 slot sums; its counter zero again on exit; dis_gn_bwd_from_sums bit-equal"""
    lib = _lib()
    hw = G.COEF_HW
    for c in G.COEF_C:
        for n in G.COEF_N:
            ab, st, gamma = G.coef_inputs(slots, n, c)
            m = hw * c
            abd, std, gad = ab.cuda(), st.reshape(-1).cuda(), gamma.cuda()
            buf, gg, gb = _coef_buf(n, c), _nan(c), _nan(c)
            counter = torch.zeros(2, dtype=torch.int32, device='cuda')
            lib.call('dis_gn_bwd_coef', std, gad, abd, slots, buf, gg, gb, counter, n, hw, c, G.EPS)
            assert int(counter[0]) == 0 and int(counter[1]) == 0
            k = buf[:n * (c + 2)].view(n, c + 2).cpu()
            s = ab.sum(dim=1)                                   # (n, 2, c), fp64 on the host
            ref = G.coef(s[:, 0], s[:, 1], st, gamma, m)
            yard = G.coef(s[:, 0], s[:, 1], st, gamma, m, dtype=F32)
            what = f'slots{slots} c{c} n{n}'
            G.check_samples(k[:, :c], ref['k1'], yard['k1'], G.TOL['coef'], family='gn_coef', out='k1', case=what)
            G.check_samples(k[:, c], ref['kx'], yard['kx'], G.TOL['coef'], family='gn_coef', out='kx', case=what)
            G.check_samples(k[:, c + 1], ref['k0'], yard['k0'], G.TOL['coef'], family='gn_coef', out='k0', case=what)
            mo = G.moments(st, m, G.EPS)
            sa = ab.abs().sum(dim=1)                            # what is summed: the slots' entries
            abs_gamma = (mo.rstd.view(n, 1) * (sa[:, 1] + mo.mean.abs().view(n, 1) * sa[:, 0])).sum(0)
            G.check_sum(gg.cpu(), ref['grad_gamma'], abs_gamma, yard['grad_gamma'], 'gn_coef', 'grad_gamma', what)
            G.check_sum(gb.cpu(), ref['grad_beta'], sa[:, 0].sum(0), yard['grad_beta'], 'gn_coef', 'grad_beta', what)
            # the one-call form: the same kernel without the counter, the parameter gradients finished by the elementwise launch
            gen = G._gen(slots, n, c, 7)
            g, x = torch.randn(n, hw, c, generator=gen).cuda(), (1.5 * torch.randn(n, hw, c, generator=gen) + 0.3).cuda()
            buf2, gg2, gb2, gx = _coef_buf(n, c), _nan(c), _nan(c), _nan(n, hw, c)
            lib.call('dis_gn_bwd_from_sums', g, x, std, gad, abd, slots, gx, gg2, gb2, buf2, n, hw, c, G.EPS, 0)
            assert torch.equal(buf2[:n * (c + 2)], buf[:n * (c + 2)]) and torch.equal(gg2, gg) and torch.equal(gb2, gb), what
            assert not bool(torch.isnan(gx).any())


# ---------------------------------------------------------------------------------------------------------------- f. from the coefficients
@pytest.mark.parametrize('case', G.SUMS_CASES)
@pytest.mark.parametrize('tag', G.SUMS_TAGS)
def test_gn_bwd_from_coefficients(tag, case):
    """gx of dis_gn_bwd_apply_coef and of dis_gn_bwd_from_sums (bit-equal), coefficients from the kernel's own dis_gn_bwd_coef on
    the exact host sums, against the direct form in fp64"""
    lib = _lib()
    n, hw, c = G.SHAPES[tag]
    m = hw * c
    d = G.inputs(case, tag)
    D = _dev(d)
    A, B, absA, absB = G.sums(d['gy'], d['x'])
    ab = torch.stack([A, B], 1).view(n, 1, 2, c).contiguous().cuda()
    buf, gg, gb = _coef_buf(n, c), _nan(c), _nan(c)
    counter = torch.zeros(2, dtype=torch.int32, device='cuda')
    lib.call('dis_gn_bwd_coef', D['st'], D['gamma'], ab, 1, buf, gg, gb, counter, n, hw, c, G.EPS)
    kref = G.coef(A, B, d['st'], d['gamma'], m)
    mo = G.moments(d['st'], m, G.EPS)
    xk = (d['x'].double() * kref['kx'].view(n, 1, 1)).abs()
    k0 = kref['k0'].abs()
    for in_act in (0, 1):
        ref = G.bwd(d['gy'], None, d['x'], d['st'], d['gamma'], 0, in_act)
        yard = G.bwd(d['gy'], None, d['x'], d['st'], d['gamma'], 0, in_act, dtype=F32)

        def allowance(sel):
            if sel is None:
                big, r = max(float(xk.max()), float(k0.max())), ref['gx']
            elif isinstance(sel, int):
                big, r = max(float(xk[sel].max()), float(k0[sel])), ref['gx'][sel]
            else:
                big, r = max(float(xk[sel].max()), float(k0.max())), ref['gx'][sel]
            return 4 * G.U32 * big / float(r.abs().max()) if float(r.abs().max()) > 0 else 0.0
        gx = _nan(n, hw, c)
        lib.call('dis_gn_bwd_apply_coef', D['gy'], D['x'], buf, gx, n, hw, c, in_act)
        buf2, gg2, gb2, gx2 = _coef_buf(n, c), _nan(c), _nan(c), _nan(n, hw, c)
        lib.call('dis_gn_bwd_from_sums', D['gy'], D['x'], D['st'], D['gamma'], ab, 1, gx2, gg2, gb2, buf2, n, hw, c, G.EPS, in_act)
        assert torch.equal(gx, gx2) and torch.equal(gg, gg2) and torch.equal(gb, gb2)
        what = f'{tag} {case} in{in_act}'
        G.check_samples(gx.cpu(), ref['gx'], yard['gx'], G.TOL['gx'], regions=_regions(case, n, hw, c), extra=allowance,
                        family='gn_from_coef', out='gx', case=what)
    abs_gamma = (mo.rstd.view(n, 1) * (absB + mo.mean.abs().view(n, 1) * absA)).sum(0)
    G.check_sum(gg.cpu(), ref['grad_gamma'], abs_gamma, yard['grad_gamma'], 'gn_from_coef', 'grad_gamma', f'{tag} {case}')
    G.check_sum(gb.cpu(), ref['grad_beta'], absA.sum(0), yard['grad_beta'], 'gn_from_coef', 'grad_beta', f'{tag} {case}')


# ---------------------------------------------------------------------------------------------------------------- g. end to end
@pytest.mark.parametrize('act,res', [(0, False), (1, True), (1, False)])
@pytest.mark.parametrize('case', ['randn', 'offset30'])
@pytest.mark.parametrize('tag', G.E2E_TAGS)
def test_group_norm_end_to_end(tag, case, act, res):
    """ops.group_norm with its own statistics, forward and through autograd, against apply + bwd in fp64 on the fp64 moments of x"""
    from depthinspace_amd import ops
    n, hw, c = G.SHAPES[tag]
    d = G.inputs(case, tag)
    xd, gd, bd = [d[k].cuda().requires_grad_(True) for k in ('x', 'gamma', 'beta')]
    rd = d['res'].cuda().requires_grad_(True) if res else None
    yd = ops.group_norm(xd, gd, bd, None, rd, act)
    yd.backward(d['gy'].cuda())
    r = d['res'] if res else None
    pre = G.apply(d['x'], d['st'], d['gamma'], d['beta'], r, act, raw=True, pre=True)
    keep = G.kink_keep(pre, act)
    assert G.excluded_share(keep) <= G.EXCLUDE_CAP
    yref = G.act_apply(pre, act, raw=True)
    ref = G.bwd(d['gy'], yref, d['x'], d['st'], d['gamma'], act, 0, raw=True)
    st32 = G.stats(d['x'], F32)[0]
    y32 = G.apply(d['x'], st32, d['gamma'], d['beta'], r, act, dtype=F32)
    yard = G.bwd(d['gy'], y32, d['x'], st32, d['gamma'], act, 0, dtype=F32)
    what = f'{tag} {case} act{act} res{int(res)}'
    G.check_samples(yd.detach().cpu(), yref, y32, G.TOL['y'], family='group_norm', out='y', case=what)
    G.check_samples(xd.grad.cpu(), ref['gx'], yard['gx'], G.TOL['gx'], keep=keep, family='group_norm', out='gx', case=what)
    if res:
        G.check_samples(rd.grad.cpu(), ref['gres'], yard['gres'], G.TOL['gres'], keep=keep, family='group_norm', out='gres', case=what)
    # the parameter gradients sum over the left-out elements too: each may sit on the other branch of SELU' (lambda against lambda alpha)
    out_g = (d['gy'].double().abs() * (G.SELU_L * G.SELU_A - G.SELU_L) * (~keep))
    mo = G.moments(d['st'], hw * c, G.EPS)
    xh = ((d['x'].double() - mo.mean_raw.view(n, 1, 1)) * mo.rstd_raw.view(n, 1, 1)).abs()
    for name, slack in (('grad_gamma', (out_g * xh).sum(dim=(0, 1))), ('grad_beta', out_g.sum(dim=(0, 1)))):
        got = (gd if name == 'grad_gamma' else bd).grad.cpu()
        G.check(got, ref[name], yard[name], G.TOL['gparam'], extra=float(slack.max()) / float(ref[name].abs().max()), family='group_norm',
                out=name, case=what)


# ---------------------------------------------------------------------------------------------------------------- h. activations
@pytest.mark.parametrize('count', G.ACT_COUNTS)
def test_act_bwd(count):
    """dis_act_bwd: one float4, one block, one float4 past it, and one block more than the 2048-block grid (every block loops)"""
    lib = _lib()
    gen = G._gen(count, 3)
    gy = torch.randn(count, generator=gen)
    y = torch.nn.functional.selu(1.5 * torch.randn(count, generator=gen))
    G.selu_edges_(y, gen)
    for act in (0, 1, 2):
        gp = _nan(count)
        lib.call('dis_act_bwd', gy.cuda(), y.cuda(), gp, act, count)
        ref = gy.double() * G.act_grad_from_out(y, act)
        yard = gy * G.act_grad_from_out(y, act, F32)
        G.check(gp.cpu(), ref, yard, G.TOL['gpre'], family='act_bwd', out='gpre', case=f'count {count} act{act}')


def _guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + numel:] == SENTINEL).all())


@pytest.mark.parametrize('c', G.ACT_LD_C)
def test_act_bwd_ld_and_bias(c):
    """channel ranges of wider buffers (every column outside them NaN), the dense gpre and the bias gradient between guards; the
    pixel counts around one block's rows and 1024 blocks' rows + 3 (every block of the bias kernel loops); c = 24: no bias form"""
    lib = _lib()
    has_bias = 256 % (c // 4) == 0
    for npix in G.act_ld_npix(c):
        for act in (0, 1, 2):
            gbuf, ybuf, gy, y, (ldg, ldy, offg, offy) = G.act_ld_inputs(npix, c, act, 5)
            gd, yd = gbuf.cuda(), ybuf.cuda()
            gv, yv = gd[:, offg:offg + c], yd[:, offy:offy + c]
            ref = gy.double() * G.act_grad_from_out(y, act)
            yard = gy * G.act_grad_from_out(y, act, F32)
            what = f'c{c} npix {npix} act{act}'
            obuf, gp = _guarded(npix * c)
            lib.call('dis_act_bwd_ld', gv, ldg, yv, ldy, gp, act, npix, c)
            assert _guards_intact(obuf, npix * c), what
            G.check(gp.view(npix, c).cpu(), ref, yard, G.TOL['gpre'], family='act_bwd_ld', out='gpre', case=what)
            if not has_bias:
                continue
            assert G.chain_length('dis_act_bwd_ld_bias', 1, npix, c) <= G.MAX_CHAIN
            ws = _nan(int(lib.fn('dis_act_bwd_ld_bias_workspace')(c)))
            obuf2, gp2 = _guarded(npix * c)
            bbuf, bias = _guarded(c)
            lib.call('dis_act_bwd_ld_bias', gv, ldg, yv, ldy, gp2, act, npix, c, bias, ws)
            assert _guards_intact(obuf2, npix * c) and _guards_intact(bbuf, c), what
            assert torch.equal(gp2, gp), what
            G.check_sum(bias.cpu(), ref.sum(0), ref.abs().sum(0), yard.sum(0), 'act_bwd_ld_bias', 'bias_grad', what)
            # the inputs are only read
            assert torch.equal(gd.view(torch.int32).cpu(), gbuf.view(torch.int32)) and torch.equal(yd.view(torch.int32).cpu(), ybuf.view(torch.int32))


@pytest.mark.parametrize('count', G.ACT_COUNTS)
def test_add_act_fwd(count):
    lib = _lib()
    a, b, big = G.add_act_inputs(count, 9)
    for act in (0, 1, 2):
        y = _nan(count)
        lib.call('dis_add_act_fwd', a.cuda(), b.cuda(), y, act, count)
        ref = G.act_apply(a.double() + b.double(), act)
        yard = G.act_apply(a + b, act)
        G.check(y.cpu(), ref, yard, G.TOL['y'], family='add_act', out='y', case=f'count {count} act{act}')
        if bool((~big).any()) and bool(big.any()):
            G.check(y.cpu(), ref, yard, G.TOL['y'], sel=~big, family='add_act', out='y', case=f'count {count} act{act} [without the 1e4 entries]')


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_unsupported_shapes_are_refused():
    lib = _lib()
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device='cuda')
    # c / 4 = 3: the backward kernels keep a channel group per thread (256 % (c / 4) == 0)
    n, hw, c = G.SHAPES['odd_cg']
    x, st, ga = z(n, hw, c), z(2 * n, dt=F64), z(c)
    wtot = lib.fn('dis_gn_bwd_workspace')(n, c)
    ws = z(wtot, dt=F64)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_gn_apply_bwd', x, None, x, st, ga, z(n, hw, c), None, z(c), z(c), ws[:2], ws[2:], n, hw, c, 0, G.EPS, 0)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_gn_bwd_res_sums', x, None, x, None, z(n, 1, 2, c, dt=F64), 1, n, hw, c, 0)
    # the from-sums family: 2 c <= 64
    n, hw, c = 1, 8, 64
    x, st, ga, ab = z(n, hw, c), z(2 * n, dt=F64), z(c), z(n, 1, 2, c, dt=F64)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_gn_bwd_res_sums', x, None, x, None, ab, 1, n, hw, c, 0)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_gn_bwd_coef', st, ga, ab, 1, z(n * (c + 2) + 4 * n * c + 2), z(c), z(c), z(2, dt=torch.int32), n, hw, c, G.EPS)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_gn_bwd_apply_coef', x, x, z(n * (c + 2) + 4 * n * c + 2), z(n, hw, c), n, hw, c, 0)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_gn_bwd_from_sums', x, x, st, ga, ab, 1, z(n, hw, c), z(c), z(c), z(n * (c + 2) + 4 * n * c + 2), n, hw, c, G.EPS, 0)
    # a count that is no multiple of 4; the bias form at c = 24 (256 % 6 != 0)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_act_bwd', z(6), z(6), z(6), 1, 6)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_add_act_fwd', z(6), z(6), z(6), 1, 6)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_act_bwd_ld_bias', z(8, 32), 32, z(8, 32), 32, z(8, 24), 1, 8, 24, z(24), z(int(lib.fn('dis_act_bwd_ld_bias_workspace')(24))))
