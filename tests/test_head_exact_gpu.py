"""The disparity head (csrc/conv2d.hip: head_fwd_kernel and head_fwd_tiled_kernel, head_gpre_kernel, head_bwd_kernel<16 / 32>,
head_reduce_kernel) against tests/head_ref.py (float64) on operands chosen so that every correct implementation returns the
same bits, whatever its order of summation:

  x   integers in [-3, 3];  w  integers in [-2, 2] times 2^-6;  b = 0.25;  offset 3.0 or 0.5;  alpha = 128.
      Every product is a multiple of 2^-6 and |z| <= 9 * 32 * 3 * 2 / 64 + 3 = 30: the pre-activation is EXACT in fp32.
  forward   what is left is alpha / (1 + expf(-z)): expf is within 1 ulp (the figure of the HIP math API's published accuracy
      table for expf; the ROCm installation this was written against ships no copy of that table to check it against), so
      t = expf(-z) is off by at most 2u (u = 2^-24), 1 + t by at most 2u t / (1 + t) + u <= 3u, the quotient by u more:
      |y - ref| <= 4u |ref| = 2^-22 |ref| PER ELEMENT - a single wrong border pixel fails.  (Measured on an MI355X: 1.12e-7
      of |ref| at the most, under half the bar.)
  backward  y is chosen, from {0, 32, 64, 96, 128}: s = y / alpha is a quarter, s (1 - s) in {0, 3/16, 1/4}, and with gy an
      integer in [-2, 2] the pre-sigmoid gradient is an integer of magnitude <= 64.  gx is then a sum of multiples of 2^-6,
      grad_w and grad_b sums of integers: all exact in fp32 while they stay below 2^24 units (asserted on the sums of the
      terms' absolute values, which bound every partial sum), so they equal the float64 reference BIT FOR BIT.

Shapes straddle the 16 rows of a forward tile and its 64 (cin 16) / 32 (cin 32) columns; (1, 257, 256) at cin 32 and
(2, 257, 256) at cin 16 are the smallest at which pixels x channel groups exceed 2048 * 256 threads, so head_bwd_kernel takes a
second trip of its grid-stride loop with the slab count at its cap, and head_reduce_kernel walks 2048 slabs; (1, 130, 128) at
cin 32 gives 520 slabs without the cap."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_ref as H

pytestmark = pytest.mark.gpu

ALPHA = 128.0
SHAPES = [(1, 1, 1), (2, 5, 3), (1, 16, 64), (1, 17, 65), (3, 33, 31), (1, 15, 33), (2, 32, 32)]
BWD_CASES = ([(cin,) + s for cin in (16, 32) for s in SHAPES] + [(32, 1, 257, 256), (16, 2, 257, 256), (32, 1, 130, 128)])


def _operands(cin, n, h, w, seed=0):
    rng = np.random.default_rng(1000 * cin + 97 * h + w + seed)
    x = rng.integers(-3, 4, (n, h, w, cin)).astype(np.float32)
    wt = (rng.integers(-2, 3, (1, cin, 3, 3)) * 2.0 ** -6).astype(np.float32)
    return rng, x, wt, np.array([0.25], np.float32)


def _forward(x, wt, b, offset, tiled):
    """dis_disp_head_fwd into a NaN-filled output, in the tiled ('1') or the grid-stride ('0') form"""
    from depthinspace_amd import lib
    n, h, w, cin = x.shape
    os.environ['DIS_HEAD_TILED'] = tiled
    try:
        y = torch.full((n, 1, h, w), float('nan'), device='cuda')
        lib.call('dis_disp_head_fwd', x, wt, b, y, n, h, w, cin, ALPHA, float(offset))
        torch.cuda.synchronize()
    finally:
        os.environ.pop('DIS_HEAD_TILED')
    return y


def _backward(x, wt, y, gy):
    """dis_disp_head_bwd with the workspace and every output NaN-filled -> (gx, grad_w, grad_b) on the host"""
    from depthinspace_amd import lib
    n, h, w, cin = x.shape
    nan = float('nan')
    gx = torch.full_like(x, nan)
    gw = torch.full((1, cin, 3, 3), nan, device='cuda')
    gb = torch.full((1,), nan, device='cuda')
    ws = torch.full((lib.fn('dis_disp_head_bwd_workspace')(n, h, w, cin),), nan, device='cuda')
    lib.call('dis_disp_head_bwd', x, wt, y, gy, gx, gw, gb, ws, n, h, w, cin, ALPHA)
    torch.cuda.synchronize()
    return gx.cpu().numpy(), gw.cpu().numpy(), gb.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize('n,h,w', SHAPES)
@pytest.mark.parametrize('cin', [16, 32])
def test_forward_per_element(cin, n, h, w):
    _, x, wt, b = _operands(cin, n, h, w)
    xd, wd, bd = (torch.from_numpy(a).cuda() for a in (x, wt, b))
    for offset in (3.0, 0.5):
        z = H.preact(x, wt, b, offset)
        assert np.array_equal(z, z.astype(np.float32).astype(np.float64)) and np.abs(z).max() <= 30.0   # exact in fp32
        ref = H.forward(x, wt, b, ALPHA, offset)
        ys = [_forward(xd, wd, bd, offset, form).cpu().numpy() for form in ('1', '0')]
        assert _same_bits(ys[0], ys[1]), 'tiled and grid-stride forms differ'
        for form, y in zip(('tiled', 'grid-stride'), ys):
            err = np.abs(y.astype(np.float64) - ref)
            assert np.all(np.isfinite(y))
            worst = float(np.max(err / ref))
            print(cin, (n, h, w), offset, form, 'worst |y - ref| / |ref| = %.3g (bar %.3g)' % (worst, 2.0 ** -22))
            assert np.all(err <= 2.0 ** -22 * np.abs(ref)), (form, offset, worst)


@pytest.mark.parametrize('cin,n,h,w', BWD_CASES)
def test_backward_bit_for_bit(cin, n, h, w):
    rng, x, wt, _ = _operands(cin, n, h, w, seed=1)
    y = (32.0 * rng.integers(0, 5, (n, 1, h, w))).astype(np.float32)
    gy = rng.integers(-2, 3, (n, 1, h, w)).astype(np.float32)
    gx, gw, gb, ax, aw, ab = H.backward(x, wt, y, gy, ALPHA, return_abs=True)
    # the condition of exactness: every sum, and every partial sum of it, is below 2^24 in units of its grid
    assert np.array_equal(gx * 64, np.round(gx * 64)) and np.array_equal(gw, np.round(gw)) and np.array_equal(gb, np.round(gb))
    assert ax.max() * 64 < 2 ** 24 and aw.max() < 2 ** 24 and ab.max() < 2 ** 24, (ax.max() * 64, aw.max(), ab.max())
    dev = [torch.from_numpy(a).cuda() for a in (x, wt, y, gy)]
    first = _backward(*dev)
    for name, got, ref in zip(('gx', 'grad_w', 'grad_b'), first, (gx, gw, gb)):
        want = ref.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref)      # (the cast rounds nothing)
        if not _same_bits(got, want):
            bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            raise AssertionError(f'{name}: {bad.size} of {got.size} elements differ, first at {int(bad[0])}: '
                                 f'{got.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}')
    for name, a, b_ in zip(('gx', 'grad_w', 'grad_b'), first, _backward(*dev)):
        assert _same_bits(a, b_), name + ' differs between two runs'


def test_saturated_pixels():
    """z = +100 and z = -100 on two pixels: expf(-100) is absorbed by 1 + t, expf(100) overflows to +inf and alpha / inf is 0:
    y is exactly alpha and exactly 0, nothing is NaN, and those pixels' s (1 - s) = 0 sends nothing back"""
    cin, n, h, w, offset = 16, 1, 9, 70, 0.5
    x = np.zeros((n, h, w, cin), np.float32)
    rng = np.random.default_rng(5)
    wt = (rng.integers(-2, 3, (1, cin, 3, 3)) * 2.0 ** -6).astype(np.float32)
    b = np.array([0.25], np.float32)
    hi, lo = (0, 0, 0), (0, 6, 66)                  # a corner of the first tile, and a pixel of the ragged second one
    x[hi][0], x[lo][1] = 1.0, 1.0
    wt[0, 0, 1, 1], wt[0, 1, 1, 1] = 100.25, -99.75   # + b - offset = +-100 exactly
    z = H.preact(x, wt, b, offset)
    assert z[hi] == 100.0 and z[lo] == -100.0 and np.abs(np.delete(z.reshape(-1), [0, 6 * w + 66])).max() < 1.0
    ref = H.forward(x, wt, b, ALPHA, offset)
    xd, wd, bd = (torch.from_numpy(a).cuda() for a in (x, wt, b))
    for form in ('1', '0'):
        y = _forward(xd, wd, bd, offset, form)
        yh = y.cpu().numpy()
        assert not np.isnan(yh).any()
        assert yh[0, 0, 0, 0] == ALPHA and yh[0, 0, 6, 66] == 0.0 and not np.signbit(yh[0, 0, 6, 66])
        rest = np.ones(yh.shape, bool)
        rest[0, 0, 0, 0] = rest[0, 0, 6, 66] = False              # (alpha * sigmoid(-100) = 4.8e-42 is not what fp32 expf gives)
        assert np.all(np.abs(yh - ref)[rest] <= 2.0 ** -22 * np.abs(ref)[rest])
        gy = np.zeros((n, 1, h, w), np.float32)
        gy[0, 0, 0, 0], gy[0, 0, 6, 66] = -2.0, 2.0
        gx, gw, gb = _backward(xd, wd, y, torch.from_numpy(gy).cuda())
        assert not gx.any() and not gw.any() and not gb.any()      # exactly zero everywhere (and no NaN)


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize('n,h,w', [(2, 37, 45), (1, 16, 64)])
def test_autograd_path_cin32(n, h, w):
    """ops.disp_head, the path the networks use, at 32 channels with random float operands against float64 torch at the
    project's bars for this operator (tests/test_net_ops_gpu.py::test_disp_head): 2e-6 forward, 1e-5 each gradient.

    x and the output gradient are POSITIVE (uniform in [0, 1) and [0.5, 1.5)), so that grad_w and grad_b are sums of terms of one
    sign.  With a zero-mean output gradient grad_b is a cancelling sum - 3330 signed terms adding up to 4.4 on (2, 37, 45) - and
    the fp32 rounding of the stored y alone (head_ref.stored_output_error: up to 4.4e-4 of grad_b there, 1.3e-5 on (1, 16, 64))
    is above a 1e-5 bar for ANY backward that starts from y, float torch's included: with randn operands this kernel's grad_b was
    2.1e-5 from float64 on (2, 37, 45), everything else within its bar.  The first assertion below states the condition on the
    float64 reference alone, before the kernel runs: the stored-output uncertainty is below a tenth of each gradient's bar (it
    is 7e-8 of the largest entry at the most with these operands)."""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(h)
    cin = 32
    x = torch.rand(n, h, w, cin, generator=g)
    wt = torch.randn(1, cin, 3, 3, generator=g) * 0.2
    b = torch.randn(1, generator=g)
    go = torch.rand(n, 1, h, w, generator=g) + 0.5
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr, br = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    y = ALPHA * torch.sigmoid(F.conv2d(xr, wr, br, padding=1) - 3.0)
    y.backward(go.double())
    inherent = H.stored_output_error(x.numpy(), wt.numpy(), y.detach().numpy(), go.numpy(), ALPHA)
    for name, e, ref in zip(('gx', 'grad_w', 'grad_b'), inherent, (xr.grad, wr.grad, br.grad)):
        assert e.max() < 0.1 * 1e-5 * float(ref.abs().max()), (name, e.max(), float(ref.abs().max()))
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, wt, b))
    yd = ops.disp_head(xd, wd, bd, ALPHA, 3.0)
    yd.backward(go.cuda())
    assert _relerr(yd, y) < 2e-6
    assert _relerr(xd.grad, xr.grad.permute(0, 2, 3, 1)) < 1e-5
    assert _relerr(wd.grad, wr.grad) < 1e-5
    assert _relerr(bd.grad, br.grad) < 1e-5
