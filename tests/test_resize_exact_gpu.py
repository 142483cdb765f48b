"""The bilinear resizes of csrc/layout_ops.hip, every entry point on every dispatch path, against tests/resize_ref.py (float64,
built from the kernels' own fp32 index / weight rule) and tests/bitexact.py (ATen's roundings).  Outputs are NaN-filled before
each call and compared on the host.

Paths.  dis_resize_bilinear_nhwc_{fwd,bwd}: c = 3 -> resize_nhwc_*_kernel<1>; c = 8 -> <4>; c = 16 -> the tiled kernels with
CG = 4 (a workgroup owns 8 rows x 64 columns); c = 32 -> tiled, CG = 8 (8 rows x 32 columns); c = 16 / 32 through tensors at a
4-byte offset -> <4> again (the tiled forms need 16-byte alignment).  The forward tiles the OUTPUT, the backward the SOURCE.
dis_resize_bilinear_planar_{fwd,bwd}: one grid-stride kernel each; the forward takes ATen's vectorised order of the four taps
when hout + wout <= 128 and its generic order otherwise.  Every backward finds its readers through resize_dst_range.

A. Bit for bit (integers in [-31, 31], power-of-two scales: every term is a multiple of one power of two and the sums of
   absolute terms stay below 2^24 such units - asserted - so ANY correct order of summation gives the reference's bits):
     align_corners=True
       (5,9,9,17)       2x up, one tile; 3 readers per source index: the backward's tables
       (9,33,17,65)     2x up.  Forward: 65 output columns = 2 full CG=8 tiles + 1 ragged column, 1 full CG=4 tile + 1 column;
                        17 rows = 2 tiles + 1 row.  Backward: 33 source columns = a CG=8 tile + 1 column, 9 rows = a tile + 1 row
       (9,65,17,129)    the same past the 64 columns of CG=4: 129 = 2 x 64 + 1 forward, 65 = 64 + 1 backward; generic ATen order
       (17,65,9,33)     2x down: every other source pixel has no reader (an all-zero table, gradient exactly 0), several tiles
       (4,3,13,17)      4x by 8x up: 7 and 15 readers, both axes raise `wide`; (3,5,17,9): rows wide, columns in tables
       (5,3,9,17)       rows in tables (3 readers), columns wide (15): the flag of one axis sends the workgroup to the general loop
       (17,9,5,3)       4x down: three of four source rows / columns unread
       (1,5,1,9) (5,1,9,1) (5,5,1,1)   extents of 1: scale 0, resize_dst_range returns the whole axis;  (6,6,6,6) identity
     align_corners=False
       (6,5,12,10)      2x up: 4 readers per source index, src clamped at 0 on the first row / column
       (8,33,16,66) (8,65,16,130) (16,66,8,33)   the tile straddles above (130 + 16 > 128: generic ATen order in the planar forward)
       (5,3,20,24)      4x by 8x up: wide;  (6,3,12,24): rows in tables, columns wide
       (20,16,5,2)      4x by 8x down;  (1,4,4,8) (4,1,1,1): extents of 1
   One launch per grid-stride kernel with more than 2048 x 256 work items, the cap of dis_ew_grid, so that the loop takes a second
   trip: (211,211,421,421) / (212,212,424,424) forward, the reversed shapes backward.

B. Per element against float64 at ratios that are no power of two (standard normal inputs), the same kernels and paths:
       forward   |y - ref|  <= 5 u forward_mag        u = 2^-24; mag = the same product on absolute values
       backward  |gx - ref| <= (T + 2) u backward_mag  T = the largest count of readers of a source pixel (rows x columns)
   DERIVED, not measured.  Forward: a tap passes through at most four roundings (its product, the inner sum, the outer product,
   the outer sum - in the nhwc association and in both ATen orders), one more u covers the second-order terms and the store.
   Backward: wy * wx, the product with the gradient, and T sequential additions: T + 1, and one more u as above.
   (7,5,40,33) (9,13,27,39): wide.  (13,67,21,100) (66,70,100,131): tables, several tiles, ragged edges; 100 + 131 > 128.
   (9,41,21,101): scale 0.4, up to 5 readers per source index on both axes: the tables full (RZ_NZ = 5), never `wide`.
   (100,67,37,13) (67,100,3,7) (30,38,15,19): down.  (2,2,7,3) (1,3,2,6): tiny.
   (5,2,29,42): with align_corners the fp32 quotients of resize_dst_range land on the wrong side of an integer here: a range
   without its rounding allowance drops a reader (tests/test_resize_ref_cpu.py works out which margins lose what).
   Largest err / (u mag) observed on an MI355X over all shapes and both align modes, recorded here and used by no assertion
   (forward against the bar of 5; backward, with the T of the shape it occurred at, against T + 2; and the largest fraction of
   the backward bar any shape used, which is reached at T = 1):
       nhwc <1>                      3.16    3.71 (T = 16, bar 18)    0.60 of the bar
       nhwc <4>, c = 8               3.16    4.24 (T = 16)            0.60
       nhwc tiled CG = 4 and CG = 8  3.16    4.50 (T = 16)            0.64
       nhwc <4>, c = 16 / 32 offset  3.16    4.50 (T = 16)            0.64   (the same bits as the tiled forms)
       planar                        3.39    3.71 (T = 16)            0.60
       planar with flow scale        2.84    -

C. align_corners=True beyond 2x down: dis_resize_bilinear_planar_fwd and dis_mf_geometry_resize equal bitexact.resize_ac, and so
   F.interpolate (tests/test_bitexact_cpu.py), bit for bit; the resized mask is `> 0.5`, strictly.

What a wrong kernel fails (part A; random integers, so a dropped or misplaced term changes the value):
   l0 / l1 swapped            (5,9,9,17): output (0,0) has src 0, l0 = 1, l1 = 0 and would read pixel 1 instead of pixel 0
   a dst range short by one   (5,9,9,17): source row 1 is read by output rows 1, 2, 3; a range that starts at 2 loses weight 1/2
                              (resize_dst_range as shipped is two indices wider than the readers on each side at these shapes)
   the last ragged column     (9,33,17,65) at c = 32 and (9,65,17,129) at c = 16: output column 64 / 128 forward and source
   of a tile skipped          column 32 / 64 backward are the only column of their tile and would keep their NaN
"""
import numpy as np
import pytest
import torch

from tests import resize_ref as RR

pytestmark = pytest.mark.gpu

U = RR.U
CAP = 2048 * 256   # threads of the largest grid dis_ew_grid hands out
NHWC_PATHS = [(3, False, '<1>'), (8, False, '<4>'), (16, False, 'tiled CG=4'), (32, False, 'tiled CG=8'),
              (16, True, '<4> c=16 offset'), (32, True, '<4> c=32 offset')]


def _dev(a, offset=False):
    """a host array on the device; offset: at an address 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    if not offset:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _nan(shape, offset=False):
    return _dev(np.full(shape, np.nan, np.float32), offset)


def _nhwc_fwd(x, shape, ac, offset=False):
    """x (n,c,hin,win) host -> (n,c,ho,wo) host through dis_resize_bilinear_nhwc_fwd"""
    from depthinspace_amd import lib
    hin, win, ho, wo = shape
    n, c = x.shape[:2]
    y = _nan((n, ho, wo, c), offset)
    lib.call('dis_resize_bilinear_nhwc_fwd', _dev(x.transpose(0, 2, 3, 1), offset), y, n, hin, win, ho, wo, c, int(ac))
    return y.cpu().numpy().transpose(0, 3, 1, 2)


def _nhwc_bwd(g, shape, ac, offset=False):
    """g (n,c,ho,wo) host -> (n,c,hin,win) host through dis_resize_bilinear_nhwc_bwd"""
    from depthinspace_amd import lib
    hin, win, ho, wo = shape
    n, c = g.shape[:2]
    gx = _nan((n, hin, win, c), offset)
    lib.call('dis_resize_bilinear_nhwc_bwd', _dev(g.transpose(0, 2, 3, 1), offset), gx, n, hin, win, ho, wo, c, int(ac))
    return gx.cpu().numpy().transpose(0, 3, 1, 2)


def _planar_fwd(x, shape, ac):
    from depthinspace_amd import lib
    hin, win, ho, wo = shape
    y = _nan(x.shape[:-2] + (ho, wo))
    lib.call('dis_resize_bilinear_planar_fwd', _dev(x), y, int(np.prod(x.shape[:-2])), hin, win, ho, wo, int(ac), 1.0, 1.0, 0)
    return y.cpu().numpy()


def _planar_bwd(g, shape, ac):
    from depthinspace_amd import lib
    hin, win, ho, wo = shape
    gx = _nan(g.shape[:-2] + (hin, win))
    lib.call('dis_resize_bilinear_planar_bwd', _dev(g), gx, int(np.prod(g.shape[:-2])), hin, win, ho, wo, int(ac))
    return gx.cpu().numpy()


FLOW_SCALE = (0.5, 0.25)


def _planar_flow(x, shape, ac):
    """what ops.resize_planar(x, size, ac, flow_scale=FLOW_SCALE) launches for x (3,2,hin,win), into a NaN-filled output: plane 0 of
    each pair times 0.5, plane 1 times 0.25"""
    from depthinspace_amd import lib
    hin, win, ho, wo = shape
    assert x.shape[:2] == (3, 2)
    y = _nan((3, 2, ho, wo))
    lib.call('dis_resize_bilinear_planar_fwd', _dev(x), y, 6, hin, win, ho, wo, int(ac), FLOW_SCALE[0], FLOW_SCALE[1], 2)
    return y.cpu().numpy()


def _same(got, ref64, what):
    """got (fp32) equals the float64 reference, which fits fp32, at every element; names the first one that differs"""
    want = ref64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref64), what + ': the reference does not fit fp32'
    assert got.shape == want.shape and got.dtype == np.float32
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)              # (a NaN - an element never written - differs from everything)
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at index {at} of {got.shape}: '
                             f'{got[at]!r} != {want[at]!r}')


def _exact_guard(shape, ac, x=None, go=None):
    """the condition under which every order of summation gives the same bits: power-of-two scales, and the sum of the absolute
    terms of every output element below 2^24 units of the finest weight product"""
    hin, win, ho, wo = shape
    unit = RR.dyadic_unit(*shape, ac)
    assert unit is not None and unit >= 2.0 ** -22, 'a scale of this shape is no power of two'
    if x is not None:
        assert RR.forward_mag(x, ho, wo, ac).max() / unit < 2 ** 24
    if go is not None:
        assert RR.backward_mag(go, hin, win, ac).max() / unit < 2 ** 24


def _ints(rng, *shape):
    return rng.integers(-31, 32, shape).astype(np.float32)


@pytest.mark.parametrize('ac,shape', [(ac, s) for ac in (True, False) for s in RR.DYADIC[ac]])
def test_bit_for_bit_on_dyadic_scales(ac, shape):
    hin, win, ho, wo = shape
    rng = np.random.default_rng(hin * 1000 + wo)
    x, go = _ints(rng, 2, 32, hin, win), _ints(rng, 2, 32, ho, wo)
    _exact_guard(shape, ac, x, go)
    y, gx = RR.forward(x, ho, wo, ac), RR.backward(go, hin, win, ac)
    for c, offset, name in NHWC_PATHS:
        _same(_nhwc_fwd(x[:, :c], shape, ac, offset), y[:, :c], f'nhwc forward {name}')
        _same(_nhwc_bwd(go[:, :c], shape, ac, offset), gx[:, :c], f'nhwc backward {name}')
    _same(_planar_fwd(x[0, :6], shape, ac), y[0, :6], 'planar forward')
    _same(_planar_bwd(go[0, :6], shape, ac), gx[0, :6], 'planar backward')
    sc = np.array(FLOW_SCALE).reshape(1, 2, 1, 1)
    xf = x[1, :6].reshape(3, 2, hin, win)
    yf = _planar_flow(xf, shape, ac)
    _same(yf, y[1, :6].reshape(3, 2, ho, wo) * sc, 'planar forward, flow scale')
    # the wrappers the networks call hand the same arguments on (autograd forward and backward)
    from depthinspace_amd import ops
    assert np.array_equal(ops.resize_planar(_dev(xf), (ho, wo), ac, flow_scale=FLOW_SCALE).cpu().numpy(), yf)
    for c in (3, 32):
        xd = _dev(x[:, :c].transpose(0, 2, 3, 1)).requires_grad_(True)
        yd = ops.resize_nhwc(xd, (ho, wo), ac)
        yd.backward(_dev(go[:, :c].transpose(0, 2, 3, 1)))
        _same(yd.detach().cpu().numpy().transpose(0, 3, 1, 2), y[:, :c], f'ops.resize_nhwc c={c}')
        _same(xd.grad.cpu().numpy().transpose(0, 3, 1, 2), gx[:, :c], f'ops.resize_nhwc backward c={c}')
    xp = _dev(x[0, :6]).requires_grad_(True)
    yp = ops.resize_planar(xp, (ho, wo), ac)
    yp.backward(_dev(go[0, :6]))
    _same(yp.detach().cpu().numpy(), y[0, :6], 'ops.resize_planar')
    _same(xp.grad.cpu().numpy(), gx[0, :6], 'ops.resize_planar backward')


@pytest.mark.parametrize('ac', [True, False])
def test_second_trip_of_every_grid_stride_loop(ac):
    """more work items than 2048 x 256 threads: the elements of the second trip sit at the end of the tensor"""
    s = RR.SECOND_TRIP[ac]
    r = RR.reverse(s)
    rng = np.random.default_rng(s[0])
    for fwd_shape, run_f, run_b, lead, per in (((3,), _planar_fwd, _planar_bwd, 'planar', 1),
                                               ((2, 8), _nhwc_fwd, _nhwc_bwd, 'nhwc <4>', 4),
                                               ((1, 3), _nhwc_fwd, _nhwc_bwd, 'nhwc <1>', 1)):
        nel = int(np.prod(fwd_shape))
        assert nel * s[2] * s[3] // per > CAP and nel * r[0] * r[1] // per > CAP
        x, go = _ints(rng, *fwd_shape, s[0], s[1]), _ints(rng, *fwd_shape, r[2], r[3])
        _exact_guard(s, ac, x=x)
        _exact_guard(r, ac, go=go)
        _same(run_f(x, s, ac), RR.forward(x, s[2], s[3], ac), lead + ' forward, second trip')
        _same(run_b(go, r, ac), RR.backward(go, r[0], r[1], ac), lead + ' backward, second trip')


def _bounded(got, ref, mag, k, what):
    err = np.abs(got.astype(np.float64) - ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    worst = RR.worst_multiple(err, mag)
    if not np.all(err <= k * U * mag):
        at = tuple(int(v) for v in np.argwhere(err > k * U * mag)[0])
        raise AssertionError(f'{what}: worst err = {worst:.2f} u mag against a bar of {k}; first at index {at} of {got.shape}: '
                             f'{got[at]!r} vs {ref[at]!r}')
    return worst


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('shape', RR.AWKWARD)
def test_per_element_at_awkward_ratios(ac, shape):
    hin, win, ho, wo = shape
    rng = np.random.default_rng(hin * 1000 + wo + 7)
    x = rng.standard_normal((2, 32, hin, win)).astype(np.float32)
    go = rng.standard_normal((2, 32, ho, wo)).astype(np.float32)
    y, gx = RR.forward(x, ho, wo, ac), RR.backward(go, hin, win, ac)
    ym, gm = RR.forward_mag(x, ho, wo, ac), RR.backward_mag(go, hin, win, ac)
    T = RR.terms(*shape, ac)
    seen = {}
    for c, offset, name in NHWC_PATHS:
        f = _bounded(_nhwc_fwd(x[:, :c], shape, ac, offset), y[:, :c], ym[:, :c], 5, f'nhwc forward {name}')
        b = _bounded(_nhwc_bwd(go[:, :c], shape, ac, offset), gx[:, :c], gm[:, :c], T + 2, f'nhwc backward {name}')
        seen['nhwc ' + name] = (f, b)
    f = _bounded(_planar_fwd(x[0, :6], shape, ac), y[0, :6], ym[0, :6], 5, 'planar forward')
    b = _bounded(_planar_bwd(go[0, :6], shape, ac), gx[0, :6], gm[0, :6], T + 2, 'planar backward')
    seen['planar'] = (f, b)
    sc = np.array(FLOW_SCALE).reshape(1, 2, 1, 1)
    f = _bounded(_planar_flow(x[1, :6].reshape(3, 2, hin, win), shape, ac), y[1, :6].reshape(3, 2, ho, wo) * sc,
                 ym[1, :6].reshape(3, 2, ho, wo) * sc, 5, 'planar forward, flow scale')
    seen['planar flow scale'] = (f, 0.0)
    for k, (f, b) in seen.items():
        print('RESIZE_B|%s|ac=%d|%s|T=%d|fwd %.3f|bwd %.3f' % (k, ac, shape, T, f, b))


# ------------------------------------------------------------------------------------------------ C: ATen's roundings
@pytest.mark.parametrize('shape', RR.ATEN_AC)
def test_planar_ac_is_aten_bit_for_bit(shape):
    from tests import bitexact as B
    hin, win, ho, wo = shape
    rng = np.random.default_rng(hin * 100 + wo)
    x = rng.standard_normal((2, 3, hin, win)).astype(np.float32)
    _same(_planar_fwd(x, shape, True), B.resize_ac(x, ho, wo).astype(np.float64), 'planar forward vs ATen')
    from depthinspace_amd import ops
    assert np.array_equal(ops.resize_planar(_dev(x), (ho, wo), True).cpu().numpy(), B.resize_ac(x, ho, wo))


def _geometry(tl, bs, h, w, seed):
    """a geometry tensor (tl,bs,h,w,slot,4) as tests/test_track_length_gpu.py::_conv3d_inputs builds it: random xyz in front of
    the camera, a 0/1 mask with holes, slot 0 all ones"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(tl, tl, bs, 3, h, w, generator=g) * 0.05
    xyz[:, :, :, 2] += 3.0
    vv, uu = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    xyz[:, :, :, 0] += (uu - w / 2) * 0.01
    xyz[:, :, :, 1] += (vv - h / 2) * 0.01
    mask = (torch.rand(tl, tl, bs, 1, h, w, generator=g) > 0.2).float()
    mask[:, 0] = 1
    return torch.cat([xyz, mask], dim=3).permute(0, 2, 4, 5, 1, 3).contiguous().numpy()


def _geom_resize(geom, ho, wo):
    from depthinspace_amd import lib
    tl, bs, hin, win = geom.shape[:4]
    out = _nan((tl, bs, ho, wo, tl, 4))
    lib.call('dis_mf_geometry_resize', _dev(geom), out, tl, bs, hin, win, ho, wo)
    return out.cpu().numpy()


def _geom_resize_ref(geom, ho, wo):
    """bitexact.resize_ac of every (slot, component) plane; the mask `> 0.5`.  -> (reference, the mask before the threshold)"""
    from tests import bitexact as B
    r = B.resize_ac(np.ascontiguousarray(geom.transpose(0, 1, 4, 5, 2, 3)), ho, wo).transpose(0, 1, 4, 5, 2, 3).copy()
    soft = r[..., 3].copy()
    r[..., 3] = (soft > np.float32(0.5)).astype(np.float32)
    return r, soft


@pytest.mark.parametrize('tl', [2, 3, 4])
@pytest.mark.parametrize('shape', RR.ATEN_AC)
def test_mf_geometry_resize_is_aten_bit_for_bit(tl, shape):
    hin, win, ho, wo = shape
    geom = _geometry(tl, 2, hin, win, seed=tl * 1000 + hin * 10 + wo)
    ref, soft = _geom_resize_ref(geom, ho, wo)
    _same(_geom_resize(geom, ho, wo), ref.astype(np.float64), f'mf_geometry_resize tl={tl}')


def test_mf_geometry_resize_second_trip():
    """tl = 4, bs = 2 at 129 x 131: 32 x 129 x 131 work items, more than 2048 x 256"""
    tl, bs, shape = 4, 2, (64, 66, 129, 131)
    assert tl * bs * tl * shape[2] * shape[3] > CAP
    geom = _geometry(tl, bs, shape[0], shape[1], seed=11)
    ref, _ = _geom_resize_ref(geom, shape[2], shape[3])
    _same(_geom_resize(geom, shape[2], shape[3]), ref.astype(np.float64), 'mf_geometry_resize, second trip')


def test_mf_geometry_resize_mask_of_exactly_one_half_is_zero():
    """6 x 6 -> 3 x 3, the quarter-resolution size the network asks for a 6 x 6 core: scale 2.5, so output row / column 1 sits
    half way between source rows / columns 2 and 3.  A mask that averages to exactly 0.5 there must come out 0: the comparison
    is strict."""
    tl, bs = 3, 2
    geom = _geometry(tl, bs, 6, 6, seed=3)
    m = np.ones((6, 6), np.float32)
    m[2, 2] = m[3, 3] = 0      # output (1,1): four taps of 1/4, two of them set           -> 0.5
    m[2, 0] = 0                # output (1,0): column 0 alone, rows 2 and 3 at 1/2 each   -> 0.5
    m[0, 3] = 0                # output (0,1): row 0 alone, columns 2 and 3 at 1/2 each   -> 0.5
    geom[..., 3] = m[None, None, :, :, None]
    ref, soft = _geom_resize_ref(geom, 3, 3)
    for at in ((1, 1), (1, 0), (0, 1)):
        assert np.all(soft[:, :, at[0], at[1]] == np.float32(0.5))
    assert np.all(soft[:, :, 2, 2] == 1) and np.all(soft[:, :, 1, 2] == 1)
    got = _geom_resize(geom, 3, 3)
    _same(got, ref.astype(np.float64), 'mf_geometry_resize, mask of exactly 0.5')
    for at in ((1, 1), (1, 0), (0, 1)):
        assert np.all(got[:, :, at[0], at[1], :, 3] == 0)
    assert np.all(got[:, :, 2, 2, :, 3] == 1) and np.all(got[:, :, 1, 2, :, 3] == 1)
