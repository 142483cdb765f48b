"""The streaming weight gradient (csrc/conv_stream_wgrad.hip) on fp32 operands, BIT FOR BIT against float64.

The method of tests/test_convb_exact_gpu.py: x and g hold small integers (tests/int_conv_ref.py: a few channels per pixel with a value of
{+-1, +-2}), so every product and every partial sum is an integer.  Each case first asserts, on the CPU, that sum |x| |g| < 2^24 for
every entry of the weight gradient - a condition on the inputs, not a tolerance.  Then the fp32 MFMA of the generic kernel, the fmaf
chains of the head form and the fp64 sums over their slabs are exact in ANY order, and gw must EQUAL (torch.equal) what float64
autograd gives for F.conv2d; a lost, doubled or misplaced term is a difference of at least 1.  Every case pins, by the tag the
dispatcher reports, the kernel it is meant to reach, and checks that memory around gw keeps a sentinel."""
import collections
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import int_conv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0   # around gw: the call owns cG_w * cX_w * k * k floats and nothing else
FILL = 1.0e6        # lanes of the wider buffers outside the channel ranges: one of them in a sum is off by far more than any entry

# cX / cG: channels in memory, cX_w / cG_w: real ones; h, w: size of x; ld / off (elements): X and G as channel ranges of wider buffers,
# called through lib.call (None: dense tensors through ops._convg_wgrad)
Case = collections.namedtuple('Case', 'id cX cX_w cG cG_w k stride h w n ranges tag')
_R = collections.namedtuple('Ranges', 'ldX xoff ldG goff')


def _c(id, cX, cX_w, cG, cG_w, k, stride, h, w, n, tag, ranges=None):
    return Case(id, cX, cX_w, cG, cG_w, k, stride, h, w, n, ranges, tag)


CASES = [
    # generic <1,1>: 2 * 13 * 11 = 286 pixels in 2 splits of 160, the second ragged (126)
    _c('c8_32', 8, 8, 32, 32, 3, 1, 13, 11, 2, R.WGRAD_GENERIC),
    # generic <1,1>: a g tile three quarters full
    _c('c32_24', 32, 32, 24, 24, 3, 1, 9, 13, 2, R.WGRAD_GENERIC),
    # generic <2,2> (no slice-pair instance for k7 s2): output 11 x 10, 330 pixels in 2 splits of 192 / 138 (no multiple of 32)
    _c('c64_64_k7s2', 64, 64, 64, 64, 7, 2, 21, 19, 3, R.WGRAD_GENERIC),
    # <2,2> with a ragged x tile: 40 channels in memory, 33 of them real - gw has 33 input channels
    _c('c33in40_64_k7s2', 40, 33, 64, 64, 7, 2, 21, 19, 3, R.WGRAD_GENERIC),
    # c8_32 with X and G as channel ranges of wider buffers
    _c('c8_32_ranges', 8, 8, 32, 32, 3, 1, 13, 11, 2, R.WGRAD_GENERIC, _R(16, 4, 48, 12)),
    # the head form: G is a 4-lane buffer with one real channel, as ops._head_stream_bwd builds it; 24 channels have no head instance
    _c('head_16', 16, 16, 4, 1, 3, 1, 13, 17, 2, R.WGRAD_HEAD),
    _c('head_32', 32, 32, 4, 1, 3, 1, 13, 17, 2, R.WGRAD_HEAD),
    _c('head_64', 64, 64, 4, 1, 3, 1, 13, 17, 2, R.WGRAD_HEAD),
    _c('head_128', 128, 128, 4, 1, 3, 1, 13, 17, 2, R.WGRAD_HEAD),
    _c('head_24_generic', 24, 24, 4, 1, 3, 1, 13, 17, 2, R.WGRAD_GENERIC),
]
CASE_IDS = [c.id for c in CASES]


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """x (n, cX_w, h, w), g (n, cG_w, hG, wG), gw: float64 integers, and the largest sum |x| |g| of an entry of gw (computed once per
    case: read-only)"""
    c = CASES[CASE_IDS.index(case_id)]
    gen = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    pad = c.k // 2
    hG, wG = (c.h + 2 * pad - c.k) // c.stride + 1, (c.w + 2 * pad - c.k) // c.stride + 1
    x = R.sparse_ints(gen, c.n, c.cX_w, c.h, c.w, R.m_of(c.cX_w, c.k))
    g = R.sparse_ints(gen, c.n, c.cG_w, hG, wG, R.m_of(c.cG_w, c.k))

    def wgrad(x_, g_):
        wt = torch.zeros(c.cG_w, c.cX_w, c.k, c.k, dtype=torch.float64, requires_grad=True)
        F.conv2d(x_, wt, None, stride=c.stride, padding=pad).backward(g_)
        return wt.grad
    return x, g, wgrad(x, g), float(wgrad(x.abs(), g.abs()).max())


def _in_buffer(t, c_mem, ld, off):
    """(n, c, h, w) float64 -> fp32 device buffer (n, h, w, ld) holding t in channels [off, off + c), zeros up to off + c_mem, FILL in
    every other lane; and the channel range [off, off + c_mem) of it"""
    n, c, h, w = t.shape
    buf = torch.full((n, h, w, ld), FILL, dtype=torch.float32)
    buf[..., off:off + c_mem] = 0
    buf[..., off:off + c] = t.permute(0, 2, 3, 1).float()
    buf = buf.cuda()
    return buf, buf[..., off:off + c_mem]


@pytest.mark.parametrize('cid', CASE_IDS)
def test_stream_wgrad_fp32_equals_fp64_on_integers(cid):
    from depthinspace_amd import lib, ops
    c = CASES[CASE_IDS.index(cid)]
    x, g, gw_ref, bound = _reference(cid)
    assert bound < 2 ** 24, bound      # a condition on the inputs, checked first
    assert float(gw_ref.abs().amax(dim=(0, 1)).min()) > 0      # every tap carries data
    hG, wG = g.shape[2:]
    ldX, xoff, ldG, goff = c.ranges if c.ranges else (c.cX, 0, c.cG, 0)
    xbuf, xd = _in_buffer(x, c.cX, ldX, xoff)
    gbuf, gd = _in_buffer(g, c.cG, ldG, goff)
    count = c.cG_w * c.cX_w * c.k * c.k
    guard = 64
    mem = torch.full((count + 2 * guard,), SENTINEL, dtype=torch.float32, device='cuda')
    gw = mem[guard:guard + count].view(c.cG_w, c.cX_w, c.k, c.k)
    pad = c.k // 2
    lib.profile_start()
    if c.ranges:
        ws = torch.empty(lib.fn('dis_convg_wgrad_workspace')(c.n, hG, wG, c.cX, c.cG, c.k), dtype=torch.float32, device='cuda')
        lib.call('dis_convg_wgrad', xbuf, ldX, xoff, c.h, c.w, c.cX, c.cX_w, gbuf, ldG, goff, hG, wG, c.cG, c.cG_w, gw, ws, c.n, c.k,
                 c.stride, pad)
    else:
        ops._convg_wgrad(xd, c.h, c.w, c.cX, c.cX_w, gd, hG, wG, c.cG, c.cG_w, gw, c.n, c.k, c.stride, pad)
    rec = [(name, tag) for (name, _, _, tag, _) in lib.profile_stop()]
    print(f'{cid}: {rec}, largest sum |x| |g| {bound:.0f}')
    assert rec == [('dis_convg_wgrad', c.tag)], rec
    got = gw.double().cpu()
    if not torch.equal(got, gw_ref):
        bad = (got != gw_ref).nonzero()
        d = (got - gw_ref)[got != gw_ref]
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(gw_ref[tuple(i)])) for i in bad[:6]]
        pytest.fail(f'gw: {bad.shape[0]} of {count} differ (differences are '
                    f'{"integers" if bool((d == d.round()).all()) else "NOT all integers"}, largest {float(d.abs().max())}); '
                    f'first (index, got, expected): {first}')
    assert bool((mem[:guard] == SENTINEL).all()) and bool((mem[guard + count:] == SENTINEL).all())
