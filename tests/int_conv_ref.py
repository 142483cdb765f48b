"""Small-integer operands and the float64 reference of tests/test_convb_exact_gpu.py: the bf16 convolution family
(csrc/conv_bf16.hip) checked BIT FOR BIT.

The kernels multiply bf16 values exactly and accumulate in fp32.  With operands that are small integers every product and every
partial sum is an integer far below 2^24 - exact in fp32 in ANY summation order (split-K partials, slabs, atomics) - and a result
that is an integer of magnitude <= 256 is exact in bf16 (8 significant bits).  The kernel must then equal the float64 reference in
every bit; a dropped, duplicated or misplaced term is a difference of at least 1.

Operands (one torch.Generator per case):
  x, go   at every pixel exactly m channels, chosen at random among the REAL channels, hold a value of {+-1, +-2}; all others 0
  w       dense integers in [-2, 2]
  bias    integers in [-8, 8]
  m       max(1, min(c, 62 // k^2)): 6 for k = 3, 2 for k = 5, 1 for k = 7, so that k^2 * m * 2 * 2 + 8 <= 256
The bound itself - conv(|x|, |w|) + |b| <= 256, and the same for the input gradient from |go| - is computed per case and asserted
before anything runs on the device: it is a condition on the inputs, not a tolerance.  tests/test_int_conv_ref_cpu.py checks the
table on the CPU (bounds, bf16 round trip, fp32 == fp64, and that the faults the method is meant to catch do change the result)."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

BOUND = 256   # integers of magnitude <= 2^8 are exact in bf16

STREAM = 'convb_fwd_kernel (bf16 streaming)'
ST128 = '128-channel stages'
SPLITK = 'split-K'
BIG = '256 x 128 tiles'
HALO = 'bf16 LDS halo)'
HALO_KC = 'column walk'
HALO_4PH = '4 phases'
PAIRS = 'conv_wgrad_bf16x3_kernel<BF> slice pairs'
WGRAD_GENERIC = 'stream_wgrad_kernel (fp32 MFMA, split-K slabs)'     # conv_stream_wgrad.hip, for fp32 and bf16 operands alike
WGRAD_HEAD = 'stream_head_wgrad_kernel (one gradient channel)'

# fwd / dgrad: substring every dis_convb_run launch tag of the forward / input-gradient call must contain (dgrad None: not pinned;
# for a phased call the recorder keeps the LAST phase's tag).  wgrad: the exact tag of the dis_convb_wgrad call; None: the layer has
# no such call (fp32 network input: dis_act_bwd_bf16_f32 + the one-pass fp32 weight-gradient kernel of conv2d.hip).
Case = collections.namedtuple('Case', 'id cin_w cin_mem cout k stride transposed h w n x_fp32 crop relu fwd dgrad wgrad')


def _c(id, cin_w, cin_mem, cout, k, stride, h, w, relu, fwd, dgrad, wgrad, n=2, x_fp32=False, transposed=False, crop=False):
    return Case(id, cin_w, cin_mem, cout, k, stride, transposed, h, w, n, x_fp32, crop, relu, fwd, dgrad, wgrad)


CASES = [
    # ---- plain streaming kernel: < 1024 output positions per image, and cin < 128 or an fp32 x or a 16-wide cout block ----
    _c('stream_in_k7s2', 2, 4, 32, 7, 2, 20, 18, True, STREAM, None, None, x_fp32=True),     # fp32 x, no input gradient
    _c('stream_k7', 32, 32, 32, 7, 1, 13, 11, False, STREAM, STREAM, PAIRS),                  # pairs k7 s1 (two tap-row groups)
    _c('stream_k5s2', 32, 32, 64, 5, 2, 21, 19, True, STREAM, STREAM, PAIRS),                 # odd sizes; pairs k5 s2
    _c('stream_k5', 64, 64, 64, 5, 1, 11, 13, False, STREAM, STREAM, PAIRS),                  # pairs k5 s1
    _c('stream_17in24_16', 17, 24, 16, 3, 1, 16, 12, True, STREAM, STREAM, PAIRS),            # 16-wide cout block; pairs k3 s1, 16 outputs
    _c('stream_32_24', 32, 32, 24, 3, 1, 9, 13, False, STREAM, STREAM, WGRAD_GENERIC),               # partial 32-wide block; generic wgrad (24 outputs)
    _c('stream_64_72', 64, 64, 72, 3, 1, 9, 13, True, STREAM, STREAM, PAIRS),                 # second 64-wide block holds 8 channels
    _c('stream_128_16', 128, 128, 16, 3, 1, 9, 7, False, STREAM, STREAM, PAIRS),              # cin >= 128 but a 16-wide cout block
    _c('stream_tiny', 32, 32, 32, 3, 1, 3, 2, True, STREAM, STREAM, PAIRS, n=3),              # 18 positions in all: one ragged tile
    _c('stream_8_32', 8, 8, 32, 3, 1, 13, 11, True, STREAM, STREAM, WGRAD_GENERIC),                  # generic wgrad (< 16 input channels)
    _c('stream_k7s2_bf16', 32, 32, 32, 7, 2, 21, 19, False, STREAM, STREAM, WGRAD_GENERIC),          # generic wgrad (k7 s2 has no pair instance)
    _c('stream_tconv_crop', 64, 64, 32, 3, 2, 8, 7, True, STREAM, STREAM, PAIRS, transposed=True, crop=True),    # 15 x 13 of 16 x 14
    _c('stream_tconv_full', 64, 64, 32, 3, 2, 8, 7, False, STREAM, STREAM, PAIRS, transposed=True),              # pairs k3 s2, x / gy swapped
    # ---- 128-channel stages: cin >= 128, bf16 x, < 1024 positions ----
    _c('st128_128_256_s2', 128, 128, 256, 3, 2, 9, 7, True, ST128, ST128, PAIRS),             # pairs k3 s2
    _c('st128_129in136', 129, 136, 64, 3, 1, 12, 10, False, ST128, STREAM, PAIRS),            # second stage: one 8-channel chunk
    _c('st128_160_32', 160, 160, 32, 3, 1, 9, 7, False, ST128, STREAM, PAIRS),                 # the 32-wide instance
    _c('splitk_512_512', 512, 512, 512, 3, 1, 8, 7, False, SPLITK, SPLITK, PAIRS),            # 36 stages in 6 splits
    _c('splitk_384_64', 384, 384, 64, 3, 1, 8, 7, True, SPLITK, STREAM, PAIRS),               # 27 stages in 4 unequal splits
    _c('splitk_256_128_k5', 256, 256, 128, 5, 1, 6, 5, False, SPLITK, SPLITK, PAIRS),         # 50 stages in 8 splits (dgrad: 25 in 4)
    # (256 -> 512 gives the 4-tap parity class 4 taps x 4 stages = 16 < 24 stages: no split-K; 1024 channels give it 32 in 5 splits)
    _c('splitk_dgrad_s2', 256, 256, 1024, 3, 2, 16, 14, True, ST128, SPLITK, PAIRS),
    # 5952 positions = 23.25 tiles of 256; 24 x 8 = 192 tiles: exactly cb_big_for's threshold
    _c('big_tiles', 128, 128, 1024, 3, 1, 32, 31, True, BIG, SPLITK, PAIRS, n=6),
    # ---- halo form: >= 1024 output positions per image ----
    _c('halo_in_k7s2', 2, 4, 32, 7, 2, 72, 80, False, HALO, None, None, x_fp32=True),          # 4 taps per k-step, fp32 x, stride 2
    _c('halo_16_16', 16, 16, 16, 3, 1, 40, 36, False, HALO, HALO, PAIRS),                     # 2 taps per k-step
    _c('halo_17in24_16', 17, 24, 16, 3, 1, 40, 36, True, HALO, HALO, PAIRS),
    _c('halo_k7', 32, 32, 32, 7, 1, 36, 40, False, HALO_KC, HALO_KC, PAIRS),                  # streamed weights, 16-row tiles, column walk
    _c('halo_k5s2', 32, 32, 64, 5, 2, 72, 70, True, HALO, HALO, PAIRS),
    _c('halo_k5', 64, 64, 64, 5, 1, 33, 37, False, HALO_KC, HALO_KC, PAIRS),                  # two chunks, ragged tiles, column walk
    _c('halo_129in136', 129, 136, 64, 3, 1, 34, 38, True, HALO, HALO, PAIRS),                 # five chunks, the last 8 channels wide
    _c('halo_tconv_crop', 64, 64, 32, 3, 2, 36, 34, True, HALO_4PH, HALO, PAIRS, transposed=True, crop=True),
    _c('halo_tconv_full', 64, 64, 32, 3, 2, 36, 34, False, HALO_4PH, HALO, PAIRS, transposed=True),
    # cb_halo_plan, 256 -> 256 k3 on 33 x 35 (bn 64): nchunk 8, nks 9, all weights 8*9*4*64*16 = 288 KB > 75 KB -> res = 0; hv = 33 >= 32
    # and 256 + 2*16 KB + 18*18*40*2 <= 75 KB -> trh = 16, HR = HC = 18, GT = 4 streamed weight groups; no column walk (k = 3)
    _c('halo_deep_t16', 256, 256, 256, 3, 1, 33, 35, True, HALO, HALO, PAIRS),
]
CASE_IDS = [c.id for c in CASES]


def m_of(c, k):
    return max(1, min(c, 62 // (k * k)))


def sparse_ints(g, n, c_real, h, w, m, c_mem=None):
    """(n, c_mem, h, w) float64: at every pixel exactly m of the first c_real channels hold a value of {+-1, +-2}; the last real
    channel is among them at the centre pixel of image 0 at least (a small map may otherwise never draw it)"""
    c_mem = c_real if c_mem is None else c_mem
    score = torch.rand(n, h, w, c_real, generator=g)
    score[0, h // 2, w // 2, c_real - 1] = 2.0
    idx = score.topk(m, dim=-1).indices
    sign = torch.randint(0, 2, idx.shape, generator=g) * 2 - 1
    mag = torch.randint(1, 3, idx.shape, generator=g)
    out = torch.zeros(n, h, w, c_mem, dtype=torch.float64)
    out.scatter_(-1, idx, (sign * mag).double())
    return out.permute(0, 3, 1, 2).contiguous()


def dense_ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def out_hw(c):
    if c.transposed:
        return (2 * c.h - 1, 2 * c.w - 1) if c.crop else (2 * c.h, 2 * c.w)
    pad = (c.k - 1) // 2
    return (c.h + 2 * pad - c.k) // c.stride + 1, (c.w + 2 * pad - c.k) // c.stride + 1


def conv_op(c, x, w, b):
    """the layer without its activation, in the dtype of its operands; x holds the REAL channels only"""
    if c.transposed:
        oh, ow = out_hw(c)
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)[..., :oh, :ow]
    return F.conv2d(x, w, b, stride=c.stride, padding=(c.k - 1) // 2)


def make_inputs(c):
    """-> x (n, cin_w, h, w), w, b, go (n, cout, oh, ow): float64 integers"""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    x = sparse_ints(g, c.n, c.cin_w, c.h, c.w, m_of(c.cin_w, c.k))
    wshape = (c.cin_w, c.cout, c.k, c.k) if c.transposed else (c.cout, c.cin_w, c.k, c.k)
    w = dense_ints(g, wshape, -2, 2)
    b = dense_ints(g, (c.cout,), -8, 8)
    oh, ow = out_hw(c)
    go = sparse_ints(g, c.n, c.cout, oh, ow, m_of(c.cout, c.k))
    return x, w, b, go


def run_ref(c, x, w, b, go, dtype=torch.float64):
    """-> y, gx, gw, gb of the layer (+ ReLU when c.relu) in `dtype`"""
    xr, wr, br = [t.to(dtype).clone().requires_grad_(True) for t in (x, w, b)]
    y = conv_op(c, xr, wr, br)
    if c.relu:
        y = F.relu(y)
    y.backward(go.to(dtype))
    return y.detach(), xr.grad, wr.grad, br.grad


Ref = collections.namedtuple('Ref', 'x w b go y gx gw gb y_bound gx_bound')


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """inputs, float64 results and the L1 bounds max(conv(|x|, |w|) + |b|), max(conv^T(|go|, |w|)) of a case (computed once, shared:
    treat as read-only)"""
    c = CASES[CASE_IDS.index(case_id)]
    x, w, b, go = make_inputs(c)
    y, gx, gw, gb = run_ref(c, x, w, b, go)
    xa = x.abs().requires_grad_(True)
    ya = conv_op(c, xa, w.abs(), b.abs())
    gxa, = torch.autograd.grad(ya, xa, go.abs())
    return Ref(x, w, b, go, y, gx, gw, gb, float(ya.detach().max()), float(gxa.max()))


def nhwc_padded(x, c_mem):
    """(n, c, h, w) -> (n, h, w, c_mem) with zero lanes behind the real channels"""
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, c_mem, dtype=x.dtype)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out
