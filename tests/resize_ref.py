"""TEST INFRASTRUCTURE: float64 reference of the bilinear resizes of csrc/layout_ops.hip (resize_nhwc_*, resize_planar_*).

The kernels share one rule for the source index and the two weights of a destination index (resize_scale / resize_src), computed
in fp32 with every operation rounded on its own (the library is built with -ffp-contract=off).  `rule` restates it in numpy fp32,
`matrix` spreads it into a dense (out x in) float64 matrix M per axis, and a resize is then two matrix products in float64:

    forward   Y  = My . X . Mx^T          backward  GX = My^T . G . Mx

`forward_mag` / `backward_mag` are the same products on absolute values (the sum of the absolute terms of every output element:
the scale of its rounding error), `terms` the largest number of destination pixels that read one source pixel.

With integer inputs and power-of-two scales every weight is a dyadic fraction and every term a multiple of one power of two:
while the sums of absolute terms stay below 2^24 such units, fp32 computes them exactly in ANY order of summation, fused or
not, and equals this reference bit for bit (`dyadic_unit` returns the unit; the tests assert the condition).
Only tests/ may import this module.
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24   # unit roundoff of fp32


# The shapes (hin, win, ho, wo) of tests/test_resize_exact_gpu.py, shared with tests/test_resize_ref_cpu.py and
# tests/test_bitexact_cpu.py so that the references are checked against torch at every shape the GPU tests rely on them.
# (which kernel path each one reaches: the docstring of tests/test_resize_exact_gpu.py)
DYADIC = {
    True: [(5, 9, 9, 17), (9, 33, 17, 65), (9, 65, 17, 129), (17, 65, 9, 33), (4, 3, 13, 17), (5, 3, 9, 17), (17, 9, 5, 3),
           (1, 5, 1, 9), (5, 1, 9, 1), (5, 5, 1, 1), (6, 6, 6, 6), (3, 5, 17, 9)],
    False: [(6, 5, 12, 10), (8, 33, 16, 66), (8, 65, 16, 130), (16, 66, 8, 33), (5, 3, 20, 24), (20, 16, 5, 2), (1, 4, 4, 8),
            (4, 1, 1, 1), (6, 3, 12, 24)],
}
SECOND_TRIP = {True: (211, 211, 421, 421), False: (212, 212, 424, 424)}   # more than 2048 * 256 outputs per launch
AWKWARD = [(7, 5, 40, 33), (13, 67, 21, 100), (100, 67, 37, 13), (67, 100, 3, 7), (9, 13, 27, 39), (66, 70, 100, 131), (2, 2, 7, 3),
           (1, 3, 2, 6), (30, 38, 15, 19), (9, 41, 21, 101), (5, 2, 29, 42)]
ATEN_AC = [(9, 13, 5, 7), (9, 13, 4, 6), (7, 5, 40, 33), (13, 67, 21, 100), (6, 6, 6, 6), (5, 5, 1, 1), (5, 9, 3, 130)]


def reverse(s):
    return (s[2], s[3], s[0], s[1])


def rule(nin, nout, ac):
    """i0, i1 (int64), l0, l1 (fp32) of every destination index 0 .. nout-1, as resize_scale / resize_src compute them"""
    dst = np.arange(nout, dtype=f32)
    if ac:
        scale = f32(nin - 1) / f32(nout - 1) if nout > 1 else f32(0)
        src = (scale * dst).astype(f32)
    else:
        scale = f32(nin) / f32(nout)
        src = (scale * (dst + f32(0.5)).astype(f32)).astype(f32)
        src = np.maximum((src - f32(0.5)).astype(f32), f32(0))
    i0 = np.minimum(src.astype(np.int64), nin - 1)      # (int)src truncates; src >= 0
    i1 = i0 + (i0 < nin - 1)
    l1 = (src - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def matrix(nin, nout, ac):
    """dense float64 (nout, nin) interpolation matrix of `rule`; where i0 == i1 the two weights accumulate"""
    i0, i1, l0, l1 = rule(nin, nout, ac)
    M = np.zeros((nout, nin), np.float64)
    d = np.arange(nout)
    np.add.at(M, (d, i0), l0.astype(np.float64))
    np.add.at(M, (d, i1), l1.astype(np.float64))
    return M


def _fwd(My, Mx, x):
    return My @ np.asarray(x, np.float64) @ Mx.T


def _bwd(My, Mx, g):
    return My.T @ np.asarray(g, np.float64) @ Mx


def forward(x, ho, wo, ac):
    """resize of x (..., hin, win) to (..., ho, wo), float64"""
    hin, win = x.shape[-2:]
    return _fwd(matrix(hin, ho, ac), matrix(win, wo, ac), x)


def backward(g, hin, win, ac):
    """gradient (..., hin, win) of the resize's input from the gradient g (..., ho, wo) of its output, float64"""
    ho, wo = g.shape[-2:]
    return _bwd(matrix(hin, ho, ac), matrix(win, wo, ac), g)


def forward_mag(x, ho, wo, ac):
    hin, win = x.shape[-2:]
    return _fwd(np.abs(matrix(hin, ho, ac)), np.abs(matrix(win, wo, ac)), np.abs(np.asarray(x, np.float64)))


def backward_mag(g, hin, win, ac):
    ho, wo = g.shape[-2:]
    return _bwd(np.abs(matrix(hin, ho, ac)), np.abs(matrix(win, wo, ac)), np.abs(np.asarray(g, np.float64)))


def terms(hin, win, ho, wo, ac):
    """the largest count of destination pixels that read one source pixel: rows times columns"""
    ty = int((matrix(hin, ho, ac) != 0).sum(axis=0).max())
    tx = int((matrix(win, wo, ac) != 0).sum(axis=0).max())
    return ty * tx


def dst_range(i, nin, nout, ac, margin=1):
    """resize_dst_range restated in fp32: the destination indices lo .. hi among which every backward kernel looks for the readers
    of source index i.  margin: what the kernel subtracts from floor(dlo) and adds to ceil(dhi) (1 as shipped)."""
    scale = (f32(nin - 1) / f32(nout - 1) if nout > 1 else f32(0)) if ac else f32(nin) / f32(nout)
    if scale <= 0:
        return 0, nout - 1
    a, b = f32(i) - f32(1), f32(i) + f32(1)
    if ac:
        dlo, dhi = f32(a / scale), f32(b / scale)
    else:
        dlo, dhi = f32(f32(f32(a + f32(0.5)) / scale) - f32(0.5)), f32(f32(f32(b + f32(0.5)) / scale) - f32(0.5))
    lo, hi = int(np.floor(dlo)) - margin, int(np.ceil(dhi)) + margin
    if not ac and i == 0:
        lo = 0
    return max(lo, 0), min(hi, nout - 1)


def readers(nin, nout, ac):
    """per source index: (first, last) destination index with a nonzero weight on it, or None where nobody reads it"""
    M = matrix(nin, nout, ac)
    out = []
    for i in range(nin):
        r = np.flatnonzero(M[:, i])
        out.append((int(r[0]), int(r[-1])) if len(r) else None)
    return out


def worst_multiple(err, mag):
    """the largest err / (u mag) over the elements that have any term (where mag == 0 a bound of k u mag demands err == 0)"""
    nz = mag > 0
    return float((err[nz] / (U * mag[nz])).max()) if nz.any() else 0.0


def _bits(M):
    """the smallest k with M * 2^k integral, or None if there is none up to 11 (an fp32 weight of a scale that is no power of two
    needs up to 24 bits and more; two axes of 11 leave a product of two weights exact in fp32 with room to spare)"""
    for k in range(12):
        s = M * 2.0 ** k
        if np.array_equal(s, np.round(s)):
            return k
    return None


def dyadic_unit(hin, win, ho, wo, ac):
    """2^-(ky + kx), the finest product of a row weight and a column weight, or None where a scale is not a power of two"""
    ky, kx = _bits(matrix(hin, ho, ac)), _bits(matrix(win, wo, ac))
    if ky is None or kx is None:
        return None
    return 2.0 ** -(ky + kx)
