"""tests/pixel_ref.py before any GPU sees it: the fp64 statements against the fp32 oracle and against the reference goldens, and the
promises of the input generators that tests/test_pixel_ops_fp64_gpu.py relies on - proved here, on the CPU, from the fp64 reference
alone.

Distances are in units of the golden tolerance of tests/test_pixel_ops_gpu.py (pixel_ref.dist: max |x - ref| / (atol + rtol |ref|)).
The fp32 oracle against fp64, found on an x86-64 host (largest over the family's cases):
  lcn           std 2.0e+1 / out 1.4e+1 on the low-contrast image (fp32 cancellation: why bar (b) exists), < 0.2 elsewhere
  photometric   fwd 0.25, bwd 0.14
  pattern_warp  fwd 2.2, bwd 2.0 at 40 x 70 and 17 x 130 (the fp32 normalisation round trip moves the sample position), 0.02 at 2 x 2
  reductions    val <= 0.12, grad <= 0.03
  smooth_loss   val 0.26, grad 0.56
  disp_to_depth fwd 0.11, bwd 0.03
  geo_loss      val 0.03, g_depth0 0.002, g_depth1 1.6 at 2 x 512 x 432 (0.1 - 0.4 at the smaller sizes)
So the oracle lies within the golden tolerance of fp64 except where fp32 itself is ill-conditioned; there the bound asserted is what
fp32 rounding explains (see each test).
"""
import os
import numpy as np
import pytest
import torch

from tests import pixel_ref as P
from tests import bitexact as B

ORA = P.oracle_ops()
F32 = torch.float32
UP = 0.37
PHOTO_EPS = {1: 0.5, 3: 0.1, 5: 0.1, 9: 0.5, 15: 0.5}


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'ops.npz'))


def oracle_dist(what, oracle, ref, atol, rtol=0.0, keep=None):
    d = P.dist(oracle, ref, atol, rtol, keep)
    print(f'oracle vs fp64  {what:<60s} {d:10.3e}')
    return d


def position_rounding(pattern, w):
    """How far an fp32 evaluation of the pattern projection may lie from fp64 through the sample position alone.  The position goes
    through p = x - disp, a = p / (w - 1), b = a - 0.5, g = 2 b, c = g + 1, ix = c (w - 1) / 2, each rounded to fp32 (2^-24
    relative): with |p|, |ix| <= w - 1, |b| <= 1/2 and |c| <= 2 inside the image that is at most (1 + 1 + 1/2 + 1 + 1) = 4.5 times
    2^-24 (w - 1) pixels, and the sample moves by that times the largest horizontal slope of the pattern."""
    pattern = P.dbl(pattern)
    return 4.5 * 2.0 ** -24 * (w - 1) * float((pattern[..., 1:] - pattern[..., :-1]).abs().max())


def under_cap(keep, what):
    share = P.excluded_share(keep)
    assert share <= P.EXCLUDE_CAP, f'{what}: {share:.4f} of the pixels within a kink margin'
    return keep


# ---------------------------------------------------------------------------------------------------------------- goldens
def test_lcn_golden(G):
    l, s = P.lcn(G['lcn_x'])
    assert P.dist(s, G['lcn_std'], 2e-5) <= 1 and P.dist(l, G['lcn_out'], 2e-4) <= 1


@pytest.mark.parametrize('name', ['mse', 'sad', 'census_mse', 'census_sad'])
@pytest.mark.parametrize('blk,eps', [(9, 0.5), (5, 0.1)])
def test_photometric_golden(G, name, blk, eps):
    v, (g,) = P.value_and_grads(lambda e: P.photometric(e, G['ph_ta'], blk, name, eps), [G['ph_es']], G['ph_go'])
    assert P.dist(v, G[f'ph_{name}_{blk}_out'], 1e-5, 1e-5) <= 1
    assert P.dist(g, G[f'ph_{name}_{blk}_grad'], 2e-6, 2e-5) <= 1


def test_pattern_loss_golden(G):
    pat = torch.from_numpy(G['pl_pat'])
    pat1 = torch.cat([pat] * 3, 1).mean(dim=1, keepdim=True)
    box = {}

    def chain(d):
        box['proj'] = P.pattern_warp(pat1, d)
        return P.weighted_mean(P.photometric(box['proj'], G['pl_im'], 9, 'census_sad', 0.5), G['pl_std'])
    v, (g,) = P.value_and_grads(chain, [G['pl_disp']])
    # (the golden projection is an fp32 result: its sample positions carry the fp32 normalisation round trip, which the golden
    # tolerance of the HIP kernel - an fp32 evaluation of the same chain - does not have to cover; found: 8.0e-6 at one pixel)
    assert P.dist(box['proj'].detach(), G['pl_proj'], 2e-6 + position_rounding(pat1, pat1.shape[-1]), 1e-5) <= 1
    assert P.dist(v, float(G['pl_val']), 1e-6, 1e-5) <= 1
    assert P.dist(g, G['pl_grad'], 1e-8, 2e-4) <= 1


def test_smooth_golden(G):
    v, (g,) = P.value_and_grads(lambda d: P.smooth_loss(d, G['sm_amb']), [G['sm_disp']])
    assert P.dist(v, float(G['sm_val']), 1e-7, 1e-5) <= 1
    assert P.dist(g, G['sm_grad'], 1e-9, 1e-4) <= 1


def test_d2d_golden(G):
    assert P.dist(P.disp_to_depth(G['d2d_in'], P.D2D_BF), G['d2d_out'], 0.0, 1e-6) <= 1


# ---------------------------------------------------------------------------------------------------------------- LCN
@pytest.mark.parametrize('kind', P.LCN_KINDS)
@pytest.mark.parametrize('radius', P.LCN_RADII)
def test_lcn_vs_oracle(radius, kind):
    """uniform and constant images: the oracle within the golden tolerance of fp64.  Low contrast: the variance 1e-4 is the
    difference of two numbers near 4, so fp32 resolves it to ~1e-6 and the std to a few per cent: asserted within 10 % of the fp64
    std everywhere (beyond that both sides would be noise and a comparison would say nothing)."""
    for (n, h, w) in P.lcn_shapes(radius):
        x = P.lcn_input(kind, n, h, w, radius)
        (rl, rs), (ol, os_) = P.lcn(x, radius, 0.05), ORA['lcn'](x, radius, 0.05)
        ds = oracle_dist(f'lcn std r{radius} {kind} {n}x{h}x{w}', os_, rs, 2e-5)
        dl = oracle_dist(f'lcn out r{radius} {kind} {n}x{h}x{w}', ol, rl, 2e-4)
        assert bool(((os_.double() - rs).abs() <= 0.1 * rs).all())
        if kind != 'lowcontrast':
            assert ds <= 1 and dl <= 1


# ---------------------------------------------------------------------------------------------------------------- photometric
@pytest.mark.parametrize('block', P.PHOTO_BLOCKS)
@pytest.mark.parametrize('name', ['mse', 'sad', 'census_mse', 'census_sad'])
def test_photometric_vs_oracle_and_kinks(name, block):
    type_id, eps = P.PHOTO_TYPES[name], PHOTO_EPS[block]
    for (n, c, h, w) in P.PHOTO_SHAPES:
        es, ta, go = P.photo_input(type_id, n, c, h, w, block)
        keep = under_cap(P.photo_keep(es, ta, block, type_id, eps), f'{name} {block} {n, c, h, w}')
        if h > 1:
            assert bool((es[:, :, : h // 2] == ta[:, :, : h // 2]).all()) and bool(keep[:, :, : h // 2].all())   # exact ties are compared
        rv, (rg,) = P.value_and_grads(lambda e: P.photometric(e, ta, block, name, eps), [es], go)
        ov, (og,) = P.value_and_grads(lambda e: ORA['photometric'](e, ta, block, name, eps), [es], go, F32)
        tag = f'{name} b{block} {n}x{c}x{h}x{w}'
        assert oracle_dist('photometric fwd ' + tag, ov, rv, 1e-5, 1e-5) <= 1
        assert oracle_dist('photometric bwd ' + tag, og, rg, 2e-6, 2e-5, keep) <= 1


# ---------------------------------------------------------------------------------------------------------------- pattern projection
@pytest.mark.parametrize('n_h_w', P.PATTERN_SHAPES)
def test_pattern_vs_oracle_and_shares(n_h_w):
    """The oracle normalises the sample position in fp32 and ATen maps it back: the position moves by a few ulps of w, and the
    sample by that times the pattern's slope - the oracle is up to 2.2 golden tolerances from fp64 at w = 70 and 130, which is why
    the GPU sweep carries bar (b) for this operator.  Bound asserted: the golden tolerance plus position_rounding()."""
    n, h, w = n_h_w
    pat, disp, go = P.pattern_input('frac', n, h, w)
    keep, clipped = P.pattern_classes(disp)
    under_cap(keep, f'pattern {n_h_w}')
    share = float(clipped.double().mean())
    assert 0.2 <= share <= 0.8, share
    assert bool((disp > 0).any()) and bool((disp < 0).any())
    rv, (rg,) = P.value_and_grads(lambda d: P.pattern_warp(pat, d), [disp], go)
    ov, (og,) = P.value_and_grads(lambda d: ORA['pattern_warp'](pat, d), [disp], go, F32)
    oracle_dist(f'pattern fwd frac {n}x{h}x{w}', ov, rv, 2e-6, 1e-5)
    oracle_dist(f'pattern bwd frac {n}x{h}x{w}', og, rg, 1e-8, 2e-4, keep)
    assert P.dist(ov, rv, 2e-6 + position_rounding(pat, w), 1e-5) <= 1
    assert bool((rg[clipped] == 0).all()) and bool((og[clipped] == 0).all())
    pat, disp, _ = P.pattern_input('int', n, h, w)
    ix = torch.arange(w, dtype=P.F64).view(1, 1, 1, w) - P.dbl(disp)
    assert bool((ix == torch.round(ix)).all()) and bool((ix == 0).any()) and bool((ix == w - 1).any())
    assert bool((ix < 0).any()) and bool((ix > w - 1).any())
    oracle_dist(f'pattern fwd int {n}x{h}x{w}', ORA['pattern_warp'](pat, disp), P.pattern_warp(pat, disp), 2e-6, 1e-5)


# ---------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize('count', P.REDUCTION_COUNTS)
def test_reductions_vs_oracle_and_kinks(count):
    t = P.reduction_input(count)
    if count > 1:
        assert bool((t['w'] == 0).any())
    assert bool((t['sgm'] == P.SGM_THRESH).any()) or count <= 3      # at least one sgm == thresh pixel (invalid: strict >)
    if count > 50:
        assert bool(((P.dbl(t['o']) - P.dbl(t['sgm']) + P.dbl(t['noise'])) == 0).any()) and bool((t['a'] == t['b']).any())
    for wkey in (None, 'w'):
        w = t[wkey] if wkey else None
        rv, (rg,) = P.value_and_grads(lambda x: P.weighted_mean(x, w), [t['x']], UP)
        ov, (og,) = P.value_and_grads(lambda x: ORA['weighted_mean'](x, w), [t['x']], UP, F32)
        assert oracle_dist(f'weighted_mean val {wkey} {count}', ov, rv, 1e-6, 1e-5) <= 1
        assert oracle_dist(f'weighted_mean grad {wkey} {count}', og, rg, 1e-8, 2e-4) <= 1
    keep = under_cap(P.l1_keep(t['a'], t['b']), f'l1 {count}')
    rv, (rg,) = P.value_and_grads(lambda a: P.l1_mean(a, t['b']), [t['a']], UP)
    ov, (og,) = P.value_and_grads(lambda a: ORA['l1_mean'](a, t['b']), [t['a']], UP, F32)
    assert oracle_dist(f'l1_mean val {count}', ov, rv, 1e-7, 1e-6) <= 1
    assert oracle_dist(f'l1_mean grad {count}', og, rg, 1e-10, 1e-6, keep) <= 1
    keep = under_cap(P.sgm_keep(t['o'], t['sgm'], t['noise']), f'sgm {count}')
    rv, (rg,) = P.value_and_grads(lambda o: P.sgm_l1(o, t['sgm'], t['noise'], P.SGM_THRESH), [t['o']], UP)
    ov, (og,) = P.value_and_grads(lambda o: ORA['sgm_l1'](o, t['sgm'], t['noise']), [t['o']], UP, F32)
    assert bool(torch.isfinite(rv))
    assert oracle_dist(f'sgm_l1 val {count}', ov, rv, 1e-7, 1e-6) <= 1
    assert oracle_dist(f'sgm_l1 grad {count}', og, rg, 1e-10, 1e-6, keep) <= 1
    assert bool((rg.reshape(-1)[t['sgm'].reshape(-1) == P.SGM_THRESH] == 0).all())


def test_sgm_l1_without_a_valid_pixel_is_not_finite():
    """what the reference does when no pixel is valid: 0 / 0 - the value and every gradient entry are NaN"""
    o, sgm, noise = torch.full((1, 1, 2, 3), 25.0), torch.full((1, 1, 2, 3), P.SGM_THRESH), torch.full((1, 1, 2, 3), 0.25)
    for fn, dt in ((lambda x: P.sgm_l1(x, sgm, noise, P.SGM_THRESH), P.F64), (lambda x: ORA['sgm_l1'](x, sgm, noise), F32)):
        v, (g,) = P.value_and_grads(fn, [o], UP, dt)
        assert not bool(torch.isfinite(v)) and not bool(torch.isfinite(g).any())


# ---------------------------------------------------------------------------------------------------------------- smoothness
@pytest.mark.parametrize('n_h_w', P.SMOOTH_SHAPES)
def test_smooth_vs_oracle_and_kinks(n_h_w):
    n, h, w = n_h_w
    disp, amb = P.smooth_input(n, h, w)
    keep = under_cap(P.smooth_keep(disp, amb), f'smooth {n_h_w}')
    t = P.smooth_terms(disp, amb)
    if h * w >= 1000:   # the ambient edges make the exponential weight matter, and both signs of the response occur
        assert float((255 * P.sobel5(P.dbl(amb))).abs().max()) > 8
        assert float((t > 0).double().mean()) > 0.2 and float((t < 0).double().mean()) > 0.2
    if h >= 8 and w >= 8:   # the flat-zero block: exact zeros of the |.| operand, compared (sign(0) = 0)
        zero = (t == 0).all(dim=1, keepdim=True)   # (a zero pixel is left out only for a neighbouring centre's kink)
        assert bool(zero.any()) and float(keep[zero].double().mean()) > 0.9
    rv, (rg,) = P.value_and_grads(lambda d: P.smooth_loss(d, amb), [disp], UP)
    ov, (og,) = P.value_and_grads(lambda d: ORA['smooth_loss'](d, amb), [disp], UP, F32)
    assert oracle_dist(f'smooth val {n}x{h}x{w}', ov, rv, 1e-7, 1e-5) <= 1
    assert oracle_dist(f'smooth grad {n}x{h}x{w}', og, rg, 1e-9, 1e-4, keep) <= 1


# ---------------------------------------------------------------------------------------------------------------- disp -> depth
@pytest.mark.parametrize('count', P.D2D_COUNTS)
def test_d2d_vs_oracle(count):
    for first in (range(len(P.D2D_VALUES)) if count == 1 else (0,)):
        disp, go = P.d2d_input(count, first)
        if count > 5:
            for v in P.D2D_VALUES:
                assert bool((disp == v).any()) or v == 1.75
        rv, (rg,) = P.value_and_grads(lambda d: P.disp_to_depth(d, P.D2D_BF), [disp], go)
        ov, (og,) = P.value_and_grads(ORA['disp_to_depth'], [disp], go, F32)
        assert oracle_dist(f'd2d fwd {count} {first}', ov, rv, 0.0, 1e-6) <= 1
        assert oracle_dist(f'd2d bwd {count} {first}', og, rg, 1e-12, 1e-5) <= 1
        assert bool((rg[disp <= 0] == 0).all()) and bool(torch.isfinite(rg).all()) and bool(torch.isfinite(rv).all())


# ---------------------------------------------------------------------------------------------------------------- flow consistency
def _geo_term(g, i, j, mode, gscale=0.7):
    h, w = g['depth'].shape[-2:]
    clamp = P.GEO_CLAMP if mode == 'sf' else None
    args = (g['flow'][(i, j)], g['R'][i], g['t'][i], g['R'][j], g['t'][j])
    ray = ORA['make_rays'](g['K'].numpy(), h, w).numpy()
    m, _ = B.flow_consistency_mask(g['K'].numpy(), ray, g['depth'][i].numpy(), g['R'][i].numpy(), g['t'][i].numpy(), g['R'][j].numpy(),
                                   g['t'][j].numpy(), g['flow'][(i, j)].numpy(), g['flow'][(j, i)].numpy(), g['amb'][i].numpy(),
                                   g['amb'][j].numpy(), primary_depth1=g['pdepth'][j].numpy() if mode == 'mf' else None)
    ref = P.geo_dir_grads(g['depth'][i], g['depth'][j], *args, g['K'], g['Kinv'], m, clamp, gscale)
    fn, box = ORA['geo_dir'](g, i, j, P.GEO_CLAMP, mode)
    ov, ogs = P.value_and_grads(fn, [g['depth'][i], g['depth'][j]], gscale, F32)
    assert np.array_equal(box['mask'].numpy(), m)     # the oracle's own mask is the bit-exact one: the same sum on both sides
    keeps = P.geo_keep(g['depth'][i], g['depth'][j], *args, g['K'], g['Kinv'], m, clamp)
    _, _, px, py = P.geo_parts(g['depth'][i], g['depth'][j], *args, g['K'], g['Kinv'])
    partial = (((px < 0) | (px > w - 1) | (py < 0) | (py > h - 1)) & (px > -1) & (px < w) & (py > -1) & (py < h))[:, None]
    return ref, (ov, ogs[0], ogs[1]), m, keeps, partial


@pytest.mark.parametrize('mode', ['mf', 'sf'])
@pytest.mark.parametrize('bs_h_w', P.GEO_SHAPES)
def test_geo_vs_oracle_and_shares(bs_h_w, mode):
    """g_depth1 at 2 x 512 x 432: the oracle is 1.6 golden tolerances from fp64 (the scattered gradient of a pixel collects up to
    ~10 taps whose weights carry the fp32 round trip of the sample position at w = 432) - bar (b) in the GPU sweep; asserted here
    within 4 golden tolerances, within 1 at the smaller sizes."""
    bs, h, w = bs_h_w
    g = P.geo_input(bs, h, w)
    seen_partial = 0
    for (i, j) in ((0, 1), (1, 0)):
        ref, ora, m, (k0, k1, active), partial = _geo_term(g, i, j, mode)
        assert 0.0 < float(m.mean()) < 1.0
        under_cap(k0, f'geo {bs_h_w} {mode} depth0')
        under_cap(k1, f'geo {bs_h_w} {mode} depth1')
        seen_partial += int((partial & (torch.from_numpy(m) > 0)).sum())
        if mode == 'sf' and h * w > 16:
            share = float(active.double().sum()) / float(m.sum())
            assert 0.05 <= share <= 0.95, share
        tag = f'{mode} {bs}x{h}x{w} {i}->{j}'
        assert oracle_dist('geo val ' + tag, ora[0], ref[0], 1e-7, 2e-5) <= 1
        for k, keep, name in ((1, k0, 'g_depth0'), (2, k1, 'g_depth1')):
            scale = float(ref[k].abs().max())
            assert scale > 0
            assert oracle_dist(f'geo {name} ' + tag, ora[k], ref[k], 2e-5 * scale, 1e-4, keep) <= (4 if h * w > 100000 else 1)
    assert seen_partial > 0    # flows that leave the image with part of their taps, inside the mask


@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_geo_empty_mask_case(mode):
    g = P.geo_input(3, 33, 41, empty=True)
    ref, ora, m, _, _ = _geo_term(g, 0, 1, mode)
    assert float(m.sum()) == 0.0
    for k in range(3):
        assert bool((ref[k] == 0).all()) and bool((ora[k] == 0).all())


@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_geo_all_terms_case_stays_under_the_cap(mode):
    bs, h, w = 3, 33, 41
    g = P.geo_input(bs, h, w, tl=3)
    pairs = [(i, j) for i in range(3) for j in range(3) if i != j] if mode == 'mf' else [(0, 1), (1, 2), (2, 0)]
    keep = torch.ones(3, bs, 1, h, w, dtype=torch.bool)
    for (i, j) in pairs:
        _, _, m, (k0, k1, _), _ = _geo_term(g, i, j, mode)
        assert 0.0 < float(m.mean()) < 1.0
        keep[i] &= k0
        keep[j] &= k1
    under_cap(keep, f'geo all {mode}')
