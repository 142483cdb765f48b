"""HIP per-pixel and loss operators (csrc/pixel_ops.hip, through the ops.* wrappers) against the plain fp64 statements of
tests/pixel_ref.py, at shapes taken from the kernels' own constants: the smallest legal image, an exact tile, one past a tile in
each direction, a long thin image, n > 1, and sizes that make every grid-stride / tile / block-slot walk loop more than once.

BARS.  For every operator and output the bar is the larger of
  (a) the tolerance tests/test_pixel_ops_gpu.py applies to the operator's golden test, atol + rtol |ref| per element, and
  (b) 4 x the fp32 CPU oracle's own distance to the fp64 reference on the same inputs, max |oracle - ref| (the max norm, in which
      tests/test_fullsize_gpu.py and test_conv_f16x2_dynamic_range state the same rule)
(pixel_ref.check).  The oracle's distance is computed here, next to the kernel's, and never depends on the kernel's output.  There
is no other tolerance in this file.  (b) decides where fp32 itself is ill-conditioned: the LCN cancellation image, pattern
projection on wide images, and single gradient entries that cancel - with (b) taken per element relative to |ref| instead of in
the max norm, ONE comparison of the sweep misses: the smoothness gradient at 1 x 4 x 5 has an entry of 4.9e-6 that is the sum of
terms of 4.6e-3 (cancellation 935 x); the kernel is 4.3e-9 off there (9e-7 of the terms, as on every other entry, the oracle
between 1e-7 and 1.2e-6 of them), which is 2.9 golden tolerances where the oracle happens to be 0.5 off at its worst entry.)

COVERAGE OF THE COMPARISON.  Forward values are compared on every pixel.  Gradients leave out the pixels whose fp64 quantity lies
within a margin of a kink (1e-3 px of a bilinear cell boundary or clip edge; 1e-4 of the operand scale of |.|, the clamp and the
sgm threshold): there fp32 and fp64 may take different branches.  At most 1 % of a case's pixels may be left out; every test
asserts it, and tests/test_pixel_ref_cpu.py proves from the fp64 reference alone that every generator stays under the cap.
Deliberate exact ties (es == ta, o - sgm + noise == 0, flat-zero disparity) are compared: sign(0) = 0 on both sides.

MEASURED (MI355X).  `kernel`, `oracle`: distance to fp64 in units of the golden tolerance (a), the largest over the family's cases
(1 or less: (a) alone holds; above 1 the oracle is as far, and (b) is the bar).  `ratio`: |kernel - fp64| / bar, the largest over all
elements of all cases - 1 would be the bar.
  family          output               cases    kernel    oracle    ratio   case of the largest ratio
  lcn             std                     75   7.7e+00   2.0e+01    0.250   r1 lowcontrast 1x2x2  (uniform / const: kernel < 0.2)
  lcn             out                     75   1.8e+00   1.4e+01    0.250   r1 lowcontrast 1x2x2
  photometric     fwd                    228   9.7e-01   2.5e-01    0.968   mse b15 2x3x1x1 (675 equal terms summed in sequence)
  photometric     bwd                    228   1.3e-01   1.4e-01    0.132   census_sad b15 2x2x41x70
  pattern_warp    fwd                     16   2.2e+00   2.2e+00    0.250   frac 1x40x70 (equal to the oracle bit for bit there)
  pattern_warp    bwd                      8   2.0e+00   2.0e+00    0.097   frac 3x40x70
  reductions      weighted_mean val       12   2.6e-03   8.2e-03    0.003   plain 257
  reductions      weighted_mean grad      12   3.9e-04   6.1e-04    0.000   weighted 257
  reductions      l1_mean val              6   2.7e-02   1.1e-01    0.027   1
  reductions      l1_mean grad             6   1.3e-02   1.3e-02    0.013   255
  reductions      sgm_l1 val               6   3.8e-02   7.1e-02    0.038   256
  reductions      sgm_l1 grad              6   2.6e-02   2.6e-02    0.026   257
  smooth_loss     val                      8   1.2e-01   2.6e-01    0.115   1x3x3
  smooth_loss     grad                     8   2.9e+00   5.6e-01    0.180   1x9x33 (2.9: the cancelling entry at 1x4x5, see BARS)
  disp_to_depth   fwd                      7   1.1e-01   1.1e-01    0.042   count 1, disp 0
  disp_to_depth   bwd                      7   1.7e-02   2.5e-02    0.011   count 524291
  geo_loss        val                     16   2.1e-02   2.4e-02    0.021   sf 2x2x2 1->0
  geo_loss        g_depth0                16   1.7e-03   1.2e-03    0.002   sf 2x512x432 0->1
  geo_loss        g_depth1                16   1.6e+00   1.6e+00    0.250   sf 2x512x432 0->1 (equal to the oracle there)
  geo_loss        all-terms val, grad      4   7.4e-02   7.4e-02    0.074   grad sf
The whole file takes 8 s on an MI355X host (76 tests), most of it the CPU's fp64 and fp32 references.
"""
import numpy as np
import pytest
import torch

from tests import pixel_ref as P

pytestmark = pytest.mark.gpu

ORA = P.oracle_ops()
F32 = torch.float32
UP = 0.37   # upstream gradient of the scalar losses (other than 1)


def cap(keep, what):
    share = P.excluded_share(keep)
    assert share <= P.EXCLUDE_CAP, f'{what}: {share:.4f} of the pixels left out of the gradient comparison'
    return keep


# ---------------------------------------------------------------------------------------------------------------- LCN
@pytest.mark.parametrize('kind', P.LCN_KINDS)
@pytest.mark.parametrize('radius', P.LCN_RADII)
def test_lcn(radius, kind):
    """tile 32 x 8, LCN_MAXR 7; reflect_idx at the smallest legal image (radius + 1); the cancellation regime of the variance"""
    from depthinspace_amd import ops
    for (n, h, w) in P.lcn_shapes(radius):
        x = P.lcn_input(kind, n, h, w, radius)
        l, s = ops.lcn(x.cuda(), radius, 0.05)
        rl, rs = P.lcn(x, radius, 0.05)
        ol, os_ = ORA['lcn'](x, radius, 0.05)
        P.check('lcn', f'std r{radius} {kind} {n}x{h}x{w}', s.cpu(), os_, rs, 2e-5)
        P.check('lcn', f'out r{radius} {kind} {n}x{h}x{w}', l.cpu(), ol, rl, 2e-4)


def test_lcn_rejects():
    from depthinspace_amd import ops, lib
    for radius, h, w in ((8, 32, 32), (5, 5, 32), (5, 32, 5), (3, 3, 3)):
        with pytest.raises(lib.DisHipError):
            ops.lcn(torch.zeros(1, 1, h, w).cuda(), radius, 0.05)


# ---------------------------------------------------------------------------------------------------------------- photometric
PHOTO_EPS = {1: 0.5, 3: 0.1, 5: 0.1, 9: 0.5, 15: 0.5}


@pytest.mark.parametrize('block', P.PHOTO_BLOCKS)
@pytest.mark.parametrize('name', ['mse', 'sad', 'census_mse', 'census_sad'])
def test_photometric(name, block, monkeypatch):
    """the general kernels at every window the ABI takes and at images narrower than the window (clamp_mult, its size == 1 branch),
    C > 1, n > 1; the census forms at 9 x 9 with one channel both through the multi-estimate kernels and the general ones"""
    from depthinspace_amd import ops
    type_id = P.PHOTO_TYPES[name]
    eps = PHOTO_EPS[block]
    for (n, c, h, w) in P.PHOTO_SHAPES:
        es, ta, go = P.photo_input(type_id, n, c, h, w, block)
        keep = cap(P.photo_keep(es, ta, block, type_id, eps), f'{name} {block} {n, c, h, w}')
        rv, (rg,) = P.value_and_grads(lambda e: P.photometric(e, ta, block, name, eps), [es], go)
        ov, (og,) = P.value_and_grads(lambda e: ORA['photometric'](e, ta, block, name, eps), [es], go, F32)
        routes = (True, False) if ops.photometric_multi_ok(1, c, block, type_id) else (False,)
        for via_multi in routes:
            monkeypatch.setattr(ops, 'PHOTO_SINGLE_VIA_MULTI', via_multi)
            e = es.cuda().requires_grad_(True)
            out = ops.photometric(e, ta.cuda(), block, type_id, eps)
            out.backward(go.cuda())
            tag = f'{name} b{block} {n}x{c}x{h}x{w}' + (' multi' if via_multi else '')
            P.check('photometric', 'fwd ' + tag, out.cpu(), ov, rv, 1e-5, 1e-5)
            P.check('photometric', 'bwd ' + tag, e.grad.cpu(), og, rg, 2e-6, 2e-5, keep)


def test_photometric_rejects_block_17():
    from depthinspace_amd import ops, lib
    x = torch.zeros(1, 1, 20, 20).cuda()
    for t in range(4):
        with pytest.raises(lib.DisHipError):
            ops.photometric(x, x, 17, t, 0.5)


# ---------------------------------------------------------------------------------------------------------------- pattern projection
@pytest.mark.parametrize('n_h_w', P.PATTERN_SHAPES)
def test_pattern_warp(n_h_w):
    """one pattern broadcast over the batch; x - disp inside cells, below 0 and above w - 1 (disparities of both signs): forward
    everywhere, grad_disp away from the cell boundaries, and EXACTLY 0 at every clipped pixel; then x - disp on exact integer
    columns, the clip edges among them: forward only"""
    from depthinspace_amd import ops
    n, h, w = n_h_w
    pat, disp, go = P.pattern_input('frac', n, h, w)
    keep, clipped = P.pattern_classes(disp)
    cap(keep, f'pattern {n_h_w}')
    rv, (rg,) = P.value_and_grads(lambda d: P.pattern_warp(pat, d), [disp], go)
    ov, (og,) = P.value_and_grads(lambda d: ORA['pattern_warp'](pat, d), [disp], go, F32)
    d = disp.cuda().requires_grad_(True)
    proj = ops.pattern_warp(pat.cuda(), d)
    proj.backward(go.cuda())
    P.check('pattern_warp', f'fwd frac {n}x{h}x{w}', proj.cpu(), ov, rv, 2e-6, 1e-5)
    P.check('pattern_warp', f'bwd frac {n}x{h}x{w}', d.grad.cpu(), og, rg, 1e-8, 2e-4, keep)
    assert bool(clipped.any()) and bool((rg[clipped] == 0).all())
    assert bool((d.grad.cpu()[clipped] == 0).all()), 'grad_disp must be exactly 0 at clipped pixels'
    pat, disp, go = P.pattern_input('int', n, h, w)
    rv = P.pattern_warp(pat, disp)
    ov = ORA['pattern_warp'](pat, disp)
    proj = ops.pattern_warp(pat.cuda(), disp.cuda())
    P.check('pattern_warp', f'fwd int {n}x{h}x{w}', proj.cpu(), ov, rv, 2e-6, 1e-5)


# ---------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize('count', P.REDUCTION_COUNTS)
def test_reductions(count):
    """dis_red_grid caps at 512 x 256 elements per pass, dis_ew_grid at 2048 x 256: one element, around one block, and one past
    each cap; weights with zeros; sgm == thresh is invalid (strict >); exact ties; an upstream gradient other than 1"""
    from depthinspace_amd import ops
    t = P.reduction_input(count)
    c = {k: v.cuda() for k, v in t.items()}
    for wkey in (None, 'w'):
        w = t[wkey] if wkey else None
        rv, (rg,) = P.value_and_grads(lambda x: P.weighted_mean(x, w), [t['x']], UP)
        ov, (og,) = P.value_and_grads(lambda x: ORA['weighted_mean'](x, w), [t['x']], UP, F32)
        x = c['x'].clone().requires_grad_(True)
        v = ops.weighted_mean(x, c[wkey] if wkey else None)
        (v * UP).backward()
        tag = f'{"weighted" if wkey else "plain"} {count}'
        P.check('reductions', 'weighted_mean val ' + tag, v.cpu(), ov, rv, 1e-6, 1e-5)
        P.check('reductions', 'weighted_mean grad ' + tag, x.grad.cpu(), og, rg, 1e-8, 2e-4)
    # l1_mean
    keep = cap(P.l1_keep(t['a'], t['b']), f'l1 {count}')
    rv, (rg,) = P.value_and_grads(lambda a: P.l1_mean(a, t['b']), [t['a']], UP)
    ov, (og,) = P.value_and_grads(lambda a: ORA['l1_mean'](a, t['b']), [t['a']], UP, F32)
    a = c['a'].clone().requires_grad_(True)
    v = ops.l1_mean(a, c['b'])
    (v * UP).backward()
    P.check('reductions', f'l1_mean val {count}', v.cpu(), ov, rv, 1e-7, 1e-6)
    P.check('reductions', f'l1_mean grad {count}', a.grad.cpu(), og, rg, 1e-10, 1e-6, keep)
    if count > 7:
        assert bool((a.grad.cpu().reshape(-1)[2::7] == 0).all())   # exact ties: sign(0) = 0
    # sgm_l1 (no golden test of its own: the l1_mean tolerances, the same reduction and the same |.|)
    keep = cap(P.sgm_keep(t['o'], t['sgm'], t['noise']), f'sgm {count}')
    rv, (rg,) = P.value_and_grads(lambda o: P.sgm_l1(o, t['sgm'], t['noise'], P.SGM_THRESH), [t['o']], UP)
    ov, (og,) = P.value_and_grads(lambda o: ORA['sgm_l1'](o, t['sgm'], t['noise']), [t['o']], UP, F32)
    o = c['o'].clone().requires_grad_(True)
    v = ops.sgm_l1(o, c['sgm'], c['noise'], P.SGM_THRESH)
    (v * UP).backward()
    P.check('reductions', f'sgm_l1 val {count}', v.cpu(), ov, rv, 1e-7, 1e-6)
    P.check('reductions', f'sgm_l1 grad {count}', o.grad.cpu(), og, rg, 1e-10, 1e-6, keep)
    if count > 50:
        assert bool((o.grad.cpu().reshape(-1)[3::50] == 0).all())   # sgm == thresh: invalid
        assert bool((o.grad.cpu().reshape(-1)[5::50] == 0).all())   # exact ties


def test_sgm_l1_no_valid_pixel():
    """The reference divides by sum(valid) = 0: value and gradient are not finite.  The kernel's are in the same class."""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(11)
    o = 20 + 10 * torch.rand(1, 1, 9, 33, generator=g)
    sgm = 20 + 10 * torch.rand(1, 1, 9, 33, generator=g)   # <= 30 everywhere
    sgm[0, 0, 0, :5] = P.SGM_THRESH
    noise = 0.25 + torch.rand(1, 1, 9, 33, generator=g)
    rv, (rg,) = P.value_and_grads(lambda x: P.sgm_l1(x, sgm, noise, P.SGM_THRESH), [o], UP)
    assert not bool(torch.isfinite(rv)) and not bool(torch.isfinite(rg).any())
    x = o.cuda().requires_grad_(True)
    v = ops.sgm_l1(x, sgm.cuda(), noise.cuda(), P.SGM_THRESH)
    (v * UP).backward()
    assert not bool(torch.isfinite(v.cpu()))
    assert torch.equal(torch.isfinite(x.grad.cpu()), torch.isfinite(rg))


# ---------------------------------------------------------------------------------------------------------------- smoothness
@pytest.mark.parametrize('n_h_w', P.SMOOTH_SHAPES)
def test_smooth_loss(n_h_w):
    """tiles 32 x 8 (forward) and 64 x 4 (backward gather); 3 x 200 x 260 is 525 forward tiles (the tile walk of smooth_kernel beyond
    its 512 workgroups), 4 x 512 x 432 is 3 584 (beyond the 2 048 of the backward); ambient edges that make the exponential weight
    matter; a flat-zero disparity block"""
    from depthinspace_amd import ops
    n, h, w = n_h_w
    disp, amb = P.smooth_input(n, h, w)
    keep = cap(P.smooth_keep(disp, amb), f'smooth {n_h_w}')
    rv, (rg,) = P.value_and_grads(lambda d: P.smooth_loss(d, amb), [disp], UP)
    ov, (og,) = P.value_and_grads(lambda d: ORA['smooth_loss'](d, amb), [disp], UP, F32)
    d = disp.cuda().requires_grad_(True)
    v = ops.smooth_loss(d, amb.cuda())
    (v * UP).backward()
    P.check('smooth_loss', f'val {n}x{h}x{w}', v.cpu(), ov, rv, 1e-7, 1e-5)
    P.check('smooth_loss', f'grad {n}x{h}x{w}', d.grad.cpu(), og, rg, 1e-9, 1e-4, keep)


def test_smooth_rejects_h2():
    from depthinspace_amd import ops, lib
    x = torch.zeros(1, 1, 2, 8).cuda()
    with pytest.raises(lib.DisHipError):
        ops.smooth_loss(x, x)


# ---------------------------------------------------------------------------------------------------------------- disp -> depth
@pytest.mark.parametrize('count', P.D2D_COUNTS)
def test_disp_to_depth(count):
    """zero, negative, 1e-30, O(1) and 1e4 disparities; the gradient is exactly 0 where disp <= 0"""
    from depthinspace_amd import ops
    for first in (range(len(P.D2D_VALUES)) if count == 1 else (0,)):
        disp, go = P.d2d_input(count, first)
        rv, (rg,) = P.value_and_grads(lambda d: P.disp_to_depth(d, P.D2D_BF), [disp], go)
        ov, (og,) = P.value_and_grads(ORA['disp_to_depth'], [disp], go, F32)
        d = disp.cuda().requires_grad_(True)
        y = ops.disp_to_depth(d, P.D2D_BF)
        y.backward(go.cuda())
        P.check('disp_to_depth', f'fwd {count} from {first}', y.cpu(), ov, rv, 0.0, 1e-6)
        P.check('disp_to_depth', f'bwd {count} from {first}', d.grad.cpu(), og, rg, 1e-12, 1e-5)
        assert bool((d.grad.cpu()[disp <= 0] == 0).all()) and bool(torch.isfinite(d.grad).all())


# ---------------------------------------------------------------------------------------------------------------- flow consistency
def _geo_term(ops, lib, B, g, i, j, mode, gscale):
    """kernel, bit-exact mask, fp64 reference and fp32 oracle of the term i -> j of a geo_input() dict"""
    h, w = g['depth'].shape[-2:]
    K, Ki = lib.host_floats(g['K'].reshape(-1)), lib.host_floats(g['Kinv'].reshape(-1))
    clamp = P.GEO_CLAMP if mode == 'sf' else None
    args = (g['flow'][(i, j)], g['R'][i], g['t'][i], g['R'][j], g['t'][j])
    d0, d1 = g['depth'][i].cuda().requires_grad_(True), g['depth'][j].cuda().requires_grad_(True)
    val, mask = ops.geo_loss_dir(d0, d1, g['flow'][(i, j)].cuda(), g['flow'][(j, i)].cuda(), g['amb'][i].cuda(), g['amb'][j].cuda(),
                                 g['pdepth'][j].cuda() if mode == 'mf' else None, g['R'][i].cuda(), g['t'][i].cuda(), g['R'][j].cuda(),
                                 g['t'][j].cuda(), K, Ki, clamp if clamp else -1.0)
    (val * gscale).backward()
    ray = ORA['make_rays'](g['K'].numpy(), h, w).numpy()
    m, _ = B.flow_consistency_mask(g['K'].numpy(), ray, g['depth'][i].numpy(), g['R'][i].numpy(), g['t'][i].numpy(), g['R'][j].numpy(),
                                   g['t'][j].numpy(), g['flow'][(i, j)].numpy(), g['flow'][(j, i)].numpy(), g['amb'][i].numpy(),
                                   g['amb'][j].numpy(), primary_depth1=g['pdepth'][j].numpy() if mode == 'mf' else None)
    assert np.array_equal(mask.cpu().numpy(), m), f'mask {i}->{j}: {float((mask.cpu().numpy() != m).mean()):.2e} of the pixels differ'
    ref = P.geo_dir_grads(g['depth'][i], g['depth'][j], *args, g['K'], g['Kinv'], m, clamp, gscale)
    fn, box = ORA['geo_dir'](g, i, j, P.GEO_CLAMP, mode)
    ov, ogs = P.value_and_grads(fn, [g['depth'][i], g['depth'][j]], gscale, F32)
    assert np.array_equal(box['mask'].numpy(), m)
    keeps = P.geo_keep(g['depth'][i], g['depth'][j], *args, g['K'], g['Kinv'], m, clamp)
    return (val.detach().cpu(), d0.grad.cpu(), d1.grad.cpu()), ref, (ov, ogs[0], ogs[1]), m, keeps


@pytest.mark.parametrize('mode', ['mf', 'sf'])
@pytest.mark.parametrize('bs_h_w', P.GEO_SHAPES)
def test_geo_loss_dir(bs_h_w, mode):
    """one direction, both ways, value and the gradients wrt depth0 and depth1 separately: the smallest image, bs = 3, a ragged
    size, and 2 x 512 x 432 = more than GEO_BLOCKS x 256 pixels (the block-slot walk); flows that leave the image (partly valid
    taps of bilin_zeros); in 'sf' the clamp active on part of the image"""
    from depthinspace_amd import ops, lib
    from tests import bitexact as B
    bs, h, w = bs_h_w
    g = P.geo_input(bs, h, w)
    for (i, j) in ((0, 1), (1, 0)):
        ker, ref, ora, m, (k0, k1, active) = _geo_term(ops, lib, B, g, i, j, mode, 0.7)
        assert 0.0 < float(m.mean()) < 1.0
        cap(k0, f'geo {bs_h_w} {mode} depth0')
        cap(k1, f'geo {bs_h_w} {mode} depth1')
        tag = f'{mode} {bs}x{h}x{w} {i}->{j}'
        P.check('geo_loss', 'val ' + tag, ker[0], ora[0], ref[0], 1e-7, 2e-5)
        for k, keep, name in ((1, k0, 'g_depth0'), (2, k1, 'g_depth1')):
            scale = float(ref[k].abs().max())
            assert scale > 0
            P.check('geo_loss', f'{name} ' + tag, ker[k], ora[k], ref[k], 2e-5 * scale, 1e-4, keep)


@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_geo_loss_dir_empty_mask(mode):
    """ambient images more than 0.01 apart: the mask is empty everywhere - value 0, both gradients exactly 0, nothing non-finite"""
    from depthinspace_amd import ops, lib
    from tests import bitexact as B
    g = P.geo_input(3, 33, 41, empty=True)
    ker, ref, ora, m, _ = _geo_term(ops, lib, B, g, 0, 1, mode, 0.7)
    assert float(m.sum()) == 0.0
    for k in range(3):
        assert bool(torch.isfinite(ker[k]).all()) and bool((ker[k] == 0).all()) and bool((ref[k] == 0).all())


@pytest.mark.parametrize('mode', ['mf', 'sf'])
def test_geo_loss_all_vs_fp64(mode):
    """the multi-term launch (three frames, directional terms sharing frames, both gradients through atomics) against the sum of
    the fp64 terms - a reference that is not another kernel of ours.  'mf': all six terms.  'sf': the cycle 0 -> 1 -> 2 -> 0 (every
    frame once as depth0 and once as depth1): the clamp adds a second kink per term, and over six terms the union of the pixels
    within the margin of one would pass the 1 % cap (1.7 %)."""
    from depthinspace_amd import ops, lib
    from tests import bitexact as B
    bs, h, w = 3, 33, 41
    g = P.geo_input(bs, h, w, tl=3)
    pairs = [(i, j) for i in range(3) for j in range(3) if i != j] if mode == 'mf' else [(0, 1), (1, 2), (2, 0)]
    gvec = torch.linspace(0.5, 1.5, len(pairs))
    ref_g, ora_g = torch.zeros(3, bs, 1, h, w, dtype=P.F64), torch.zeros(3, bs, 1, h, w)
    keep = torch.ones(3, bs, 1, h, w, dtype=torch.bool)
    ref_v, ora_v = [], []
    for k, (i, j) in enumerate(pairs):
        _, ref, ora, m, (k0, k1, _) = _geo_term(ops, lib, B, g, i, j, mode, float(gvec[k]))
        ref_v.append(ref[0]); ora_v.append(ora[0])
        ref_g[i] += ref[1]; ref_g[j] += ref[2]
        ora_g[i] += ora[1]; ora_g[j] += ora[2]
        keep[i] &= k0; keep[j] &= k1
    cap(keep, f'geo all {mode}')
    K, Ki = lib.host_floats(g['K'].reshape(-1)), lib.host_floats(g['Kinv'].reshape(-1))
    depth = g['depth'].cuda().requires_grad_(True)
    flows = [(g['flow'][(i, j)].cuda(), g['flow'][(j, i)].cuda()) for (i, j) in pairs]
    vals = ops.geo_loss_all(depth, g['amb'].cuda(), g['pdepth'].cuda() if mode == 'mf' else None, g['R'].cuda(), g['t'].cuda(), K, Ki,
                            P.GEO_CLAMP if mode == 'sf' else -1.0, pairs, flows)
    (vals * gvec.cuda()).sum().backward()
    P.check('geo_loss', f'all-terms val {mode}', vals.cpu(), torch.stack(ora_v), torch.stack(ref_v), 1e-7, 2e-5)
    scale = float(ref_g.abs().max())
    P.check('geo_loss', f'all-terms grad {mode}', depth.grad.cpu(), ora_g, ref_g, 2e-5 * scale, 1e-4, keep)
