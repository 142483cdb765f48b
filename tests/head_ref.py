"""TEST INFRASTRUCTURE: float64 numpy reference of the disparity head (csrc/conv2d.hip: head_fwd_kernel, head_fwd_tiled_kernel,
head_gpre_kernel, head_bwd_kernel, head_reduce_kernel; reference model/networks.py's Conv2d(cin, 1, 3, padding=1) followed by
alpha * sigmoid(. - offset)).  Layouts are the kernels': x (n, h, w, cin) NHWC, w (1, cin, 3, 3), y / gy (n, 1, h, w).
tests/test_head_ref_cpu.py compares it with torch autograd in float64.  Only tests/ may import this module."""
import numpy as np


def _taps(h, w):
    """(ky, kx, output rows, output columns, input rows, input columns) of the 3x3 taps at padding 1: output pixel (oy, ox) reads
    input pixel (oy + ky - 1, ox + kx - 1) where that lies inside the image"""
    for ky in range(3):
        for kx in range(3):
            oy0, oy1 = max(0, 1 - ky), min(h, h + 1 - ky)
            ox0, ox1 = max(0, 1 - kx), min(w, w + 1 - kx)
            if oy0 < oy1 and ox0 < ox1:
                yield (ky, kx, slice(oy0, oy1), slice(ox0, ox1), slice(oy0 + ky - 1, oy1 + ky - 1),
                       slice(ox0 + kx - 1, ox1 + kx - 1))


def preact(x, w, b, offset):
    """z (n, h, w) = conv3x3_pad1(x, w) + b - offset"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, cin = x.shape
    assert w.shape == (1, cin, 3, 3)
    z = np.zeros((n, h, wd))
    for ky, kx, oy, ox, iy, ix in _taps(h, wd):
        z[:, oy, ox] += x[:, iy, ix, :] @ w[0, :, ky, kx]
    return z + (float(np.asarray(b, np.float64).reshape(-1)[0]) - float(offset))


def forward(x, w, b, alpha, offset):
    """y (n, 1, h, w) = alpha * sigmoid(z), evaluated without overflow on either side"""
    z = preact(x, w, b, offset)
    e = np.exp(-np.abs(z))
    s = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return (float(alpha) * s)[:, None]


def gpre(y, gy, alpha):
    """the pre-sigmoid gradient as the kernels define it, from the forward's OUTPUT: s = y / alpha, gy * alpha * s * (1 - s)"""
    s = np.asarray(y, np.float64) / float(alpha)
    return np.asarray(gy, np.float64) * float(alpha) * s * (1.0 - s)


def backward_from_gpre(x, w, g):
    """-> gx (n, h, w, cin), gw (1, cin, 3, 3), gb (1,) of the 3x3 convolution from its output gradient g (n, h, w)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, cin = x.shape
    g = np.asarray(g, np.float64).reshape(n, h, wd)
    gx, gw = np.zeros_like(x), np.zeros_like(w)
    for ky, kx, oy, ox, iy, ix in _taps(h, wd):
        gx[:, iy, ix, :] += g[:, oy, ox, None] * w[0, :, ky, kx]
        gw[0, :, ky, kx] = np.einsum('nyx,nyxc->c', g[:, oy, ox], x[:, iy, ix, :])
    return gx, gw, np.array([g.sum()])


def backward(x, w, y, gy, alpha, return_abs=False):
    """-> gx, gw, gb.  return_abs: also the same three sums over the ABSOLUTE values of their terms (what bounds every partial
    sum of them, in any order)"""
    g = gpre(y, gy, alpha)
    out = backward_from_gpre(x, w, g)
    if return_abs:
        out += backward_from_gpre(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(g))
    return out


def stored_output_error(x, w, y, gy, alpha):
    """What the fp32 ROUNDING OF THE STORED y alone can do to (gx, gw, gb): the backward starts from s = y / alpha, y is kept in
    fp32, and d gpre / dy = gy (1 - 2 s), so every pixel's gpre is uncertain by |gy| |1 - 2 s| ulp32(y) / 2 whatever the kernel
    does afterwards.  Returned: those uncertainties carried through the convolution's backward with absolute values - the
    worst case, from the float64 reference alone.  A relative bar on a gradient means something only where this is far below it
    (a signed, cancelling sum such as grad_b under a zero-mean gy is not such a place)."""
    y = np.asarray(y, np.float64)
    d = np.abs(np.asarray(gy, np.float64)) * np.abs(1.0 - 2.0 * y / float(alpha)) * 0.5 * np.spacing(np.abs(y).astype(np.float32))
    return backward_from_gpre(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), d)
