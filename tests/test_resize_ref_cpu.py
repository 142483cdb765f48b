"""CPU: tests/resize_ref.py (the float64 reference of the bilinear resize kernels, built from the kernels' own fp32 index / weight
rule) against torch, at every shape tests/test_resize_exact_gpu.py uses it at.

  * power-of-two scales, integer inputs: the reference equals F.interpolate in fp32 and in fp64 BIT FOR BIT, forward and
    through autograd, in both align modes - so on those shapes "equal to the reference" is "equal to torch".
  * align_corners=True: the rule equals tests/bitexact.py's lerp_idx (ATen's compute_source_index_and_lambda) exactly, and at
    the awkward shapes fp32 torch stays inside the per-element bounds the GPU tests hold the kernels to.
  * align_corners=False at the awkward shapes: torch forms the source position with other roundings than the kernels (one ulp of
    src at some columns: 13 x 67 -> 21 x 100, columns 24 and 48), so it is held to the forward bound plus the weight difference
    that three roundings of a source position can make: delta = 3u (hin + win) per weight, two weights per axis.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bitexact as B
from tests import resize_ref as RR

U = RR.U
DYADIC_CASES = ([(ac, s) for ac in (True, False) for s in RR.DYADIC[ac]]
                + [(ac, s) for ac in (True, False) for s in (RR.SECOND_TRIP[ac], RR.reverse(RR.SECOND_TRIP[ac]))])


def _torch(x, go, ho, wo, ac):
    xr = torch.from_numpy(x).clone().requires_grad_(True)
    y = F.interpolate(xr, size=(ho, wo), mode='bilinear', align_corners=ac)
    y.backward(torch.from_numpy(go))
    return y.detach().numpy(), xr.grad.numpy()


@pytest.mark.parametrize('ac,shape', DYADIC_CASES)
def test_reference_is_torch_bit_for_bit_on_dyadic_scales(ac, shape):
    hin, win, ho, wo = shape
    rng = np.random.default_rng(hin * 1000 + wo)
    lead = (1, 2) if hin > 200 else (2, 3)
    x = rng.integers(-31, 32, lead + (hin, win)).astype(np.float32)
    go = rng.integers(-31, 32, lead + (ho, wo)).astype(np.float32)
    unit = RR.dyadic_unit(hin, win, ho, wo, ac)
    assert unit is not None and unit >= 2.0 ** -23
    assert RR.forward_mag(x, ho, wo, ac).max() / unit < 2 ** 24 and RR.backward_mag(go, hin, win, ac).max() / unit < 2 ** 24
    y, gx = RR.forward(x, ho, wo, ac), RR.backward(go, hin, win, ac)
    for a in (y, gx):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)       # (fits fp32: the cast rounds nothing)
    ty, tgx = _torch(x, go, ho, wo, ac)
    assert np.array_equal(ty, y.astype(np.float32)) and np.array_equal(tgx, gx.astype(np.float32))
    dy, dgx = _torch(x.astype(np.float64), go.astype(np.float64), ho, wo, ac)
    assert np.array_equal(dy, y) and np.array_equal(dgx, gx)


AC_SHAPES = sorted(set(RR.DYADIC[True] + [RR.SECOND_TRIP[True], RR.reverse(RR.SECOND_TRIP[True])] + RR.AWKWARD + RR.ATEN_AC))


@pytest.mark.parametrize('shape', AC_SHAPES)
def test_rule_is_lerp_idx(shape):
    """(where l1 == 0 the second tap carries no weight: lerp_idx names i0 again for equal sizes, the kernels name i0 + 1)"""
    for nin, nout in ((shape[0], shape[2]), (shape[1], shape[3])):
        i0, i1, l0, l1 = RR.rule(nin, nout, True)
        j0, j1, m0, m1 = B.lerp_idx(nin, nout)
        assert np.array_equal(i0, j0) and np.array_equal(l0, m0) and np.array_equal(l1, m1)
        assert l0.dtype == np.float32 and l1.dtype == np.float32
        assert np.array_equal(i1[l1 != 0], j1[l1 != 0])
        assert i1.max() <= nin - 1 and i0.min() >= 0


def test_matrix_rows_and_terms():
    """the matrix of the rule: rows sum to 1 (up to the rounding of 1 - l1); a source index of a 2x upsample has 3 readers with
    align_corners (src = d / 2) and 4 without (src = d / 2 - 1 / 4), a 4x / 8x one 7 / 15; `terms` is rows times columns"""
    for ac in (True, False):
        for nin, nout in ((5, 9), (13, 21), (100, 37), (1, 4), (4, 1), (6, 6)):
            M = RR.matrix(nin, nout, ac)
            assert M.shape == (nout, nin) and np.all(M >= 0) and np.abs(M.sum(axis=1) - 1).max() <= U
    assert RR.terms(5, 9, 9, 17, True) == 9 and RR.terms(4, 3, 13, 17, True) == 7 * 15
    assert RR.terms(6, 5, 12, 10, False) == 16 and RR.terms(17, 9, 5, 3, True) == 1 and RR.terms(5, 5, 1, 1, True) == 1
    assert RR.dyadic_unit(13, 67, 21, 100, True) is None and RR.dyadic_unit(5, 9, 9, 17, True) == 0.25


def _covered(nin, nout, ac, margin):
    return all(r is None or (lo <= r[0] and r[1] <= hi)
               for r, (lo, hi) in zip(RR.readers(nin, nout, ac), (RR.dst_range(i, nin, nout, ac, margin) for i in range(nin))))


def test_dst_range_covers_every_reader_and_what_a_narrower_one_would_miss():
    """resize_dst_range (restated in RR.dst_range) never leaves out a destination index that reads the source index, at every
    axis of every shape the GPU tests use and at all sizes up to 40 x 40.  Its margin of one index on each side is spare at these
    sizes: without it (margin 0) the range still covers.  One index narrower than that (margin -1: floor(dlo) + 1 .. ceil(dhi) - 1,
    which is exact in real arithmetic) the fp32 rounding of (i -+ 1) / scale loses a reader at 5 -> 29 and 2 -> 42 with
    align_corners, the axes of the awkward shape (5,2,29,42), and one more index narrower (margin -2) loses one on every
    upsampling axis, the power-of-two ones of part A included - so the GPU tests fail for a range that is too narrow by one."""
    axes = set()
    for ac in (True, False):
        for s in RR.DYADIC[ac] + RR.AWKWARD + [RR.SECOND_TRIP[ac], RR.reverse(RR.SECOND_TRIP[ac])]:
            axes |= {(s[0], s[2], ac), (s[1], s[3], ac)}
        axes |= {(nin, nout, ac) for nin in range(1, 41) for nout in range(1, 41)}
    for nin, nout, ac in sorted(axes):
        assert _covered(nin, nout, ac, 1) and _covered(nin, nout, ac, 0), (nin, nout, ac)
    assert not _covered(5, 29, True, -1) and not _covered(2, 42, True, -1)
    for ac, nin, nout in ((True, 5, 9), (True, 3, 17), (False, 6, 12), (False, 3, 24)):
        assert _covered(nin, nout, ac, -1) and not _covered(nin, nout, ac, -2)


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('shape', RR.AWKWARD)
def test_torch_fp32_is_within_the_bounds_at_awkward_ratios(ac, shape):
    hin, win, ho, wo = shape
    rng = np.random.default_rng(hin * 1000 + wo)
    x = rng.standard_normal((2, 3, hin, win)).astype(np.float32)
    go = rng.standard_normal((2, 3, ho, wo)).astype(np.float32)
    ty, tgx = _torch(x, go, ho, wo, ac)
    ey = np.abs(ty - RR.forward(x, ho, wo, ac))
    mag = RR.forward_mag(x, ho, wo, ac)
    if ac:
        egx = np.abs(tgx - RR.backward(go, hin, win, ac))
        gmag = RR.backward_mag(go, hin, win, ac)
        T = RR.terms(hin, win, ho, wo, ac)
        print(shape, 'fwd %.2f u mag, bwd %.2f u mag (T = %d)' % (RR.worst_multiple(ey, mag), RR.worst_multiple(egx, gmag), T))
        assert np.all(ey <= 5 * U * mag)
        assert np.all(egx <= (T + 2) * U * gmag)
    else:
        allow = 2 * 3 * U * (hin + win) * float(np.abs(x).max())
        print(shape, 'fwd: %.3f of the allowance' % (np.maximum(ey - 5 * U * mag, 0) / allow).max())
        assert np.all(ey <= 5 * U * mag + allow)
