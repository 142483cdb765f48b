"""Conv3D (csrc/conv3d_knn.hip: select, the MFMA forward, the class-ordered backward with its per-block parameter-gradient slabs)
through its RAW entry points against the plain float64 statement of tests/conv3d_ref.py, at the shapes where its index
arithmetic can go wrong, and on the second trip of its wave loops.

BARS.  An element passes when |kernel - fp64| <= max((a), 4 max |fp32 reference - fp64|) (tests/pixel_ref.check), where (a) is
the tolerance of test_conv3d_golden as an absolute bar: 2e-5 max|ref| for y and agg, 5e-5 max|ref| for grad_wf (with a base in
the rows: of max|base + ref|), 1e-4 max|ref| for each of the five parameter gradients.  The fp32 reference is conv3d_ref.conv3d
evaluated in float32 on the CPU; its distance never depends on the kernel's output.  There is no other tolerance in part 1.
Before every launch y, agg, the parameter gradients and the workspace are filled with NaN: an unwritten output row or slab fails.

COVERAGE OF THE COMPARISON.  Forward values are compared on every pixel.  The upstream gradient is zero on the output pixels
with a float64 pre-activation inside 4e-6 of its layer's largest (SELU' jumps at 0): at most 5 % of a case's output pixels;
tests/test_conv3d_ref_cpu.py proves the cap for every case from the reference alone.

PART 1, edge shapes, at tl 2, 3, 4, stride 1 and 2, ids from the selection and random distinct ids:
    h x w     bs     what it reaches
    1 x 1     1, 5   2 ... 20 output pixels: less than one 16-pixel group, a full group and a remainder; 8 of 9 taps padded
    1 x 7     2      a single row / column; at stride 1 the classes cy >= 1 / cx >= 1 are empty (no launch)
    7 x 1     2
    2 x 2     1      every class holds at most one pixel per image
    3 x 3     1
    5 x 7     3      odd sizes: at stride 2 the last window is centred on the last row / column
    13 x 9    2
    6 x 8     2      even size at stride 2 (the last window ends inside the map)
    12 x 14   2      the shape of the golden tests; groups straddle image boundaries
    40 x 36   2      hundreds of blocks and slabs, still one group per wave
and, at 5 x 7, bs 3, the range cases: one feature row x 1e4 ('outlier'); all features x 1e-6 on a geometry x 100 ('tiny').
'outlier' is compared FORWARD ONLY: the kink margin is 4e-6 of the layer's largest pre-activation, which the outlier sets, so
the margin would cover the ordinary pixels' whole range (tests/test_conv3d_ref_cpu.py measures that share: it is far above the cap).

PART 2, the second trip of the wave loops.  conv3d_fwd_kernel runs at most 1 024 blocks and conv3d_bwd2_kernel at most C3D_CAP =
768 per class launch, 4 waves of 16 pixels each: a wave takes a second group only beyond 65 536 output pixels (forward) or
49 152 per class (backward) - in every full-size training step, and in no other test.  A launch beyond both is compared with
its own one-sample slices, which take one group per wave (the regime part 1 compares with float64): y, agg and grad_wf bit for
bit (pixels are independent; a gradient row receives at most one add per class launch, in launch order), the parameter
gradients to 1e-4 of the largest entry of the float64 sum of the slices' results.

MEASURED (MI355X).  `kernel`, `fp32 ref`: the largest distance to float64 over the family's comparisons in units of (a);
`ratio`: the largest |kernel - fp64| / bar over all elements of all comparisons - 1 would be the bar.
  cases    output             n     kernel   fp32 ref    ratio   case of the largest ratio
  edge     y                132    3.1e-02    1.9e-02    0.031   1x1 bs1 tl2 s2 random
  edge     agg              132    2.5e-02    1.2e-02    0.025   3x3 bs1 tl2 s2 select
  edge     grad_wf          132    1.5e-02    6.6e-03    0.015   2x2 bs1 tl2 s2 select
  edge     g:dense1_w       132    4.2e-03    1.3e-01    0.004   40x36 bs2 tl2 s2 select
  edge     g:dense1_b       132    4.9e-03    4.5e-03    0.005   13x9 bs2 tl4 s2 select
  edge     g:dense2_w       132    7.4e-03    6.7e-03    0.007   2x2 bs1 tl2 s2 select
  edge     g:dense2_b       132    4.4e-03    3.6e-03    0.004   12x14 bs2 tl2 s2 random
  edge     g:w              132    5.3e-03    5.8e-03    0.005   1x7 bs2 tl2 s1 select
  edge     base+grad_wf     132    4.1e-03    3.0e-03    0.004   40x36 bs2 tl3 s1 random
  outlier  y                 12    2.1e-02    1.4e-02    0.021   5x7 bs3 tl3 s2 select
  outlier  agg               12    3.6e-02    9.2e-03    0.036   5x7 bs3 tl3 s2 select
  tiny     y                 12    1.7e-02    1.7e-02    0.017   5x7 bs3 tl2 s1 random
  tiny     agg               12    9.9e-03    1.1e-02    0.010   5x7 bs3 tl3 s2 select
  tiny     grad_wf           12    6.1e-03    5.2e-03    0.006   5x7 bs3 tl3 s1 random
  tiny     g:dense1_w        12    4.1e-03    2.9e-02    0.004   5x7 bs3 tl4 s2 select
  tiny     g:dense1_b        12    4.1e-03    3.0e-03    0.004   5x7 bs3 tl2 s2 random
  tiny     g:dense2_w        12    4.2e-03    4.3e-03    0.004   5x7 bs3 tl2 s2 select
  tiny     g:dense2_b        12    2.6e-03    2.9e-03    0.003   5x7 bs3 tl3 s2 select
  tiny     g:w               12    2.4e-03    6.3e-03    0.002   5x7 bs3 tl2 s1 select
  tiny     base+grad_wf      12    6.2e-03    5.4e-03    0.006   5x7 bs3 tl3 s1 random
The kernels sit where the fp32 reference sits, 3e-7 to 7e-7 of the largest entry from float64.  One comparison of the sweep
missed when this file was written: y of 'tiny' was 28 to 138 tolerances away (6e-4 to 3e-3 of the largest output) in all 12
cases, because the output SELU formed exp(x) - 1 from a rounded exp - an absolute error of 1e-7, against outputs of 4e-5.
conv3d_fwd_kernel now takes the series of expm1 below |x| = 2^-6 (selu_out); the figures above are with it.
Second trip: bit-identical y, agg and grad_wf; parameter gradients 1.7e-7 to 6.6e-7 of the largest entry from the fp64 sum of
the slices (bar 1e-4).  tl 3 is not thinned: the whole file takes 6 s on an MI355X host (226 tests, 1 180 comparisons), most of
it the CPU's fp64 and fp32 references.
"""
import pytest
import torch

from tests import conv3d_ref as R
from tests import pixel_ref as P

pytestmark = pytest.mark.gpu

NAN = float('nan')
BARS = {'y': 2e-5, 'agg': 2e-5, 'grad_wf': 5e-5}   # parameter gradients: 1e-4
FWD_PIXELS_PER_TRIP = 1024 * 4 * 16                # the forward's block cap x waves x pixels of a group
BWD_PIXELS_PER_TRIP = 768 * 4 * 16                 # C3D_CAP likewise, per class launch


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device='cuda')


def raw_forward(geom, wf, params, idx, stride, with_agg=True):
    from depthinspace_amd import ops
    tl, bs, h, w = geom.shape[:4]
    ho, wo = idx.shape[2:4]
    y = _nan(tl, bs, ho, wo, R.C)
    if not with_agg:
        ops.lib.call('dis_conv3d_knn_fwd', geom, wf, *params, idx, y, tl, bs, h, w, stride)
        return y
    agg = _nan(tl, bs, ho, wo, R.C)
    ops.lib.call('dis_conv3d_knn_fwd_agg', geom, wf, *params, idx, y, agg, tl, bs, h, w, stride)
    return y, agg


def raw_backward(geom, wf, params, idx, y, agg, gy, grad_wf, stride):
    """dis_conv3d_knn_bwd_det: ADDS to the rows of grad_wf; -> the 1632 parameter gradients"""
    from depthinspace_amd import ops
    tl, bs, h, w = geom.shape[:4]
    n = ops.lib.fn('dis_conv3d_knn_bwd_det_workspace')(tl, bs, h, w, stride)
    assert n > 0
    ws, gp = _nan(n), _nan(1632)
    ops.lib.call('dis_conv3d_knn_bwd_det', geom, wf, *params, idx, y, agg, gy, grad_wf, gp, ws, tl, bs, h, w, stride)
    return gp


def _amax(x):
    return float(x.abs().max())


class Checks(object):
    """pixel_ref.check for every output of a case before the first miss is raised: a case reports all its figures"""

    def __init__(self):
        self.missed = []

    def __call__(self, what, kernel, f32, ref, atol):
        try:
            P.check('conv3d', what, kernel, f32, ref, atol)
        except AssertionError as e:
            self.missed.append(str(e))

    def done(self):
        assert not self.missed, '\n'.join(self.missed)


def compare(c, tag, backward=True):
    """forward and backward of the case c through the raw entry points against c.ref (fp64), bars scaled with c.f32"""
    check, out = Checks(), None
    try:
        out = _compare(c, tag, backward, check)
    except AssertionError as e:   # (a bitwise assertion: reported with the figures collected so far)
        check.missed.append(str(e))
    check.done()
    return out


def _compare(c, tag, backward, check):
    geom, wf, idx, gy = c.geom.cuda(), c.wf.cuda(), c.idx.cuda(), c.gy.cuda()
    params = [p.cuda() for p in c.params]
    y, agg = raw_forward(geom, wf, params, idx, c.stride)
    for k, v in (('y', y), ('agg', agg)):
        check(f'{k} {tag}', v.cpu(), c.f32[k], c.ref[k], BARS[k] * _amax(c.ref[k]))
    assert torch.equal(raw_forward(geom, wf, params, idx, c.stride, with_agg=False), y), 'dis_conv3d_knn_fwd: another y'
    if not backward:
        return y, None, None
    runs = []
    for rep in range(2):   # zeroed rows, twice: bit-identical
        g = torch.zeros_like(wf)
        runs.append((g, raw_backward(geom, wf, params, idx, y, agg, gy, g, c.stride)))
    (g0, gp0), (g1, gp1) = runs
    assert torch.equal(g0, g1) and torch.equal(gp0, gp1), 'the backward does not repeat bit for bit'
    check(f'grad_wf {tag}', g0.cpu(), c.f32['grad_wf'], c.ref['grad_wf'], BARS['grad_wf'] * _amax(c.ref['grad_wf']))
    for k in R.PARAMS:
        a, b = R.GP_SLICES[k]
        check(f'g:{k} {tag}', gp0[a:b].cpu().view(R.PARAM_SHAPES[k]), c.f32[k], c.ref[k], 1e-4 * _amax(c.ref[k]))
    # a base in the rows: the result is base + gradient, and a row no (pixel, neighbour) names keeps its bits
    gb = c.base.cuda()
    gpb = raw_backward(geom, wf, params, idx, y, agg, gy, gb, c.stride)
    want = c.base.double() + c.ref['grad_wf']
    check(f'base+grad_wf {tag}', gb.cpu(), c.base + c.f32['grad_wf'], want, BARS['grad_wf'] * _amax(want))
    assert torch.equal(gpb, gp0), 'the parameter gradients depend on what grad_wf held'
    idle = (c.ref['grad_wf'] == 0).all(dim=-1) & (c.f32['grad_wf'] == 0).all(dim=-1)
    assert torch.equal(gb.cpu()[idle], c.base[idle]), 'a row without a gradient was rewritten'
    return y, g0, gp0


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('tl', R.TLS)
@pytest.mark.parametrize('h,w,bs', R.EDGE_SHAPES)
def test_selection_bit_exact_at_edge_shapes(h, w, bs, tl, stride):
    """ops.conv3d_select == tests/bitexact.py's selection bit for bit: holes (slot 0 valid), pixels masked in every slot and
    nothing valid at all (every key ties at the fill value: nth_element's order decides, border candidates are chosen)"""
    from depthinspace_amd import ops
    for k, kind in enumerate(R.MASK_KINDS):
        xyz, mask = R.geometry(tl, bs, h, w, P._gen(17, tl, bs, h, w, stride, k), kind)
        want = R.select_ids(xyz, mask, stride)
        got = ops.conv3d_select(R.to_geom(xyz, mask).cuda(), stride)
        assert tuple(got.shape) == (tl, bs) + R.out_dims(h, w, stride) + (9,)
        assert torch.equal(got.cpu(), want), f'{kind}: {float((got.cpu() != want).float().mean()):.2e} of the ids differ'


@pytest.mark.parametrize('ids', R.ID_SOURCES)
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('tl', R.TLS)
@pytest.mark.parametrize('h,w,bs', R.EDGE_SHAPES)
def test_edge_shape(h, w, bs, tl, stride, ids):
    from depthinspace_amd import ops
    c = R.make_case(tl, bs, h, w, stride, ids)
    assert c.share <= R.KINK_CAP
    if ids == 'select':
        assert torch.equal(ops.conv3d_select(c.geom.cuda(), stride).cpu(), c.idx)
    compare(c, f'{h}x{w} bs{bs} tl{tl} s{stride} {ids}')


@pytest.mark.parametrize('h,w,bs,tl,stride,ids,rng', R.range_cases())
def test_range_case(h, w, bs, tl, stride, ids, rng):
    c = R.make_case(tl, bs, h, w, stride, ids, rng, grads=True)
    compare(c, f'{rng} {h}x{w} bs{bs} tl{tl} s{stride} {ids}', backward=rng in R.RANGES_WITH_BACKWARD)


@pytest.mark.parametrize('stride', [1, 2])
def test_autograd_path_equals_the_raw_calls(stride):
    """ops.conv3d_knn (what the network calls): y, the feature gradient and the five parameter gradients are the raw entry
    points' bits"""
    from depthinspace_amd import ops
    h, w, bs = R.RANGE_SHAPE
    tl = 3
    c = R.make_case(tl, bs, h, w, stride, 'random')
    y_raw, g_raw, gp_raw = compare(c, f'autograd {h}x{w} bs{bs} tl{tl} s{stride}')
    wf = c.wf.cuda().requires_grad_(True)
    ps = dict(zip(R.PARAMS, [p.cuda().requires_grad_(True) for p in c.params]))
    y = ops.conv3d_knn(c.geom.cuda(), wf, *[ps[k] for k in R.PARAMS], c.idx.cuda(), stride)
    y.backward(c.gy.cuda())
    assert torch.equal(y.detach(), y_raw) and torch.equal(wf.grad, g_raw)
    for k in R.PARAMS:
        a, b = R.GP_SLICES[k]
        assert torch.equal(ps[k].grad.reshape(-1), gp_raw[a:b]), k


@pytest.mark.parametrize('stride,h,w,bs', [(1, 180, 180, 8), (2, 360, 360, 4)])
def test_second_trip_of_the_wave_loops(stride, h, w, bs):
    """the launch takes several groups per wave, its one-sample slices one: see PART 2"""
    tl = 2
    ho, wo = R.out_dims(h, w, stride)
    cn = 3 if stride == 1 else 2
    per_class = tl * ((ho + cn - 1) // cn) * ((wo + cn - 1) // cn)      # the largest class, per sample
    assert tl * bs * ho * wo > FWD_PIXELS_PER_TRIP >= tl * ho * wo
    assert bs * per_class > BWD_PIXELS_PER_TRIP >= per_class
    g = torch.Generator(device='cuda').manual_seed(1000 + stride)
    geom = torch.randn(tl, bs, h, w, tl, 4, device='cuda', generator=g) * 0.05
    geom[..., 2] += 3.0
    geom[..., 0] += ((torch.arange(w, device='cuda') - w / 2) * 0.01).view(1, 1, 1, w, 1)
    geom[..., 1] += ((torch.arange(h, device='cuda') - h / 2) * 0.01).view(1, 1, h, 1, 1)
    wf = torch.randn(tl, bs, h, w, tl, R.C, device='cuda', generator=g)
    idx = torch.rand(tl, bs, ho, wo, 9 * tl, device='cuda', generator=g).argsort(dim=-1)[..., :9].to(torch.uint8).contiguous()
    gy = torch.randn(tl, bs, ho, wo, R.C, device='cuda', generator=g)
    base = torch.randn(tl, bs, h, w, tl, R.C, device='cuda', generator=g)
    params = [p.cuda() for p in R.make_params(torch.Generator().manual_seed(stride))]
    y, agg = raw_forward(geom, wf, params, idx, stride)
    gw = base.clone()
    gp = raw_backward(geom, wf, params, idx, y, agg, gy, gw, stride)
    assert bool(torch.isfinite(gp).all())
    total = torch.zeros(1632, dtype=torch.float64, device='cuda')
    for b in range(bs):
        one = lambda t: t[:, b:b + 1].contiguous()
        geom_b, wf_b, idx_b = one(geom), one(wf), one(idx)
        y_b, agg_b = raw_forward(geom_b, wf_b, params, idx_b, stride)
        assert torch.equal(y_b, y[:, b:b + 1]), f'y of sample {b}'
        assert torch.equal(agg_b, agg[:, b:b + 1]), f'agg of sample {b}'
        gw_b = one(base)
        total += raw_backward(geom_b, wf_b, params, idx_b, y_b, agg_b, one(gy), gw_b, stride).double()
        assert torch.equal(gw_b, gw[:, b:b + 1]), f'grad_wf of sample {b}'
    for k in R.PARAMS:
        a, e = R.GP_SLICES[k]
        err, scale = float((gp[a:e].double() - total[a:e]).abs().max()), float(total[a:e].abs().max())
        print(f'second trip s{stride} g:{k}: {err / scale:.3e} of the largest entry')
        assert err <= 1e-4 * scale, (k, err, scale)
