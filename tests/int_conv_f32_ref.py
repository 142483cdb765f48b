"""Wide-integer operands, the float64 reference and the case table of tests/test_convg_exact_gpu.py: the fp32-storage streaming
convolutions (csrc/conv_gen.hip, the channel slices and weight-gradient forms of csrc/conv2d.hip / conv_f16x2.hip /
conv_stream_wgrad.hip behind ops.convg / ops.convg_transposed) checked BIT FOR BIT.

tests/int_conv_ref.py does this for bf16 storage with operands |v| <= 2.  Under the default two-term fp16 split of the fp32 path a
value is h1 + h2 (after a power-of-two scale that takes its block's maximum into [2^14, 2^15)) and a product is a1 b1 + a1 b2 + a2 b1;
with |v| <= 2 every h2 is zero and the two cross terms are never exercised.  Here a sprinkle of entries is +-2049 = 2^11 + 1 (12
significant bits: h1 = 2048 s, h2 = s; in the three-term bf16 split 2048 + 1 + 0), placed so that NO product has two wide factors:

  x    dense integers in [-2, 2]; wide only in image 0 and in even input channels   (the 2-in-4 stem: channel 0)
  go   dense integers in [-2, 2]; wide only in image 1 and in even output channels
  w    dense integers in [-2, 2]; wide only at (odd output channel, odd input channel)
  b    integers in [-8, 8]

forward: a wide x (even ci) meets w[:, even ci], narrow.  Input gradient: a wide go (even co) meets w[even co, :], narrow.  Weight
gradient: wide x and wide go live in different images.  So the dropped a2 b2 term is identically zero, both splits and plain fp32 are
exact, and every fp32 partial sum is an integer multiple of the launch's power-of-two unit.  With the L1 bounds below 2^24 - asserted
per case before anything runs on a device: conditions on the inputs, not tolerances - every sum is exact in ANY order, and y, gx, gw,
gb must EQUAL float64.  A lost first-plane term is a difference of at least 1, a lost second-plane term exactly the low part of a
wide value.  Every case needs n >= 2.

One wide value of x (go) is forced into the last pixel - a border pixel of the last row - of the last even channel, which lies in the
last chunk of 32 (16) real channels; one wide value of w is forced into the first and the last tap of (last odd output channel, last
odd input channel).  (A channel count of 32 m + 1 leaves the last chunk without an odd channel: w's forced value then sits in the
chunk before it.)  tests/test_int_conv_f32_ref_cpu.py checks the table on the CPU: bounds, fp32 == fp64, the emulated two-term
products, and that the faults the method is meant to catch - second-plane ones included - do change the result."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

from tests.int_conv_ref import WGRAD_GENERIC, dense_ints, nhwc_padded, out_hw, conv_op   # noqa: F401  (shared with the bf16 table)

BOUND = 2 ** 24     # integers below 2^24 (in units of the launch's power-of-two scale) are exact in fp32
WIDE = 2049.0       # 2^11 + 1

# ---- kernel tags (DIS_TAG in the dispatchers) ----
FP32 = 'convg_fwd_kernel (fp32 MFMA streaming)'            # cin < 32 under either split (the tap-packed form has the same tag)
G2 = 'convg2_fwd_kernel (f16x2 streaming)'
G2_SK = 'convg2_fwd_kernel (f16x2 streaming, split-K)'
G2_BIG = 'convg2_fwd_kernel (f16x2 streaming, 256 x 128 tiles)'
G2_BIG_SK = 'convg2_fwd_kernel (f16x2 streaming, 256 x 128 tiles, split-K)'
H2 = 'convh2_kernel (f16x2 LDS halo)'                      # streamed weights
H2_RES = 'convh2_kernel (f16x2 LDS halo, resident weights)'
H2_KC = 'convh2_kernel (f16x2 LDS halo, column walk)'
H2_4PH = 'convh2_kernel (f16x2 LDS halo, 4 phases)'
H2_4PH_RES = 'convh2_kernel (f16x2 LDS halo, 4 phases, resident weights)'
G3 = 'convg3_fwd_kernel (bf16x3 streaming)'
SL2 = 'conv_f16x2_kernel<32,32,GEN> slices'
SL3 = 'conv_bf16x3_kernel<32,32,GEN> slices'
# weight gradient: (entry point, tag)
PAIRS2 = ('dis_convg_wgrad', 'conv_wgrad_f16x2_kernel slice pairs')
PAIRS3 = ('dis_convg_wgrad', 'conv_wgrad_bf16x3_kernel slice pairs')
GENERIC = ('dis_convg_wgrad', WGRAD_GENERIC)
ONE_STEM = ('dis_conv2d_wgrad', 'conv_wgrad_kernel (fp32 MFMA)')              # the one-pass kernels of conv2d.hip: x dense and
ONE2_16_16 = ('dis_conv2d_wgrad_bf16x3', 'conv_wgrad_f16x2_kernel<16,16>')    # dis_conv2d_wgrad_workspace(cin_mem, cout, k, stride) >= 0
ONE2_32_16 = ('dis_conv2d_wgrad_bf16x3', 'conv_wgrad_f16x2_kernel<32,16>')
ONE3_16_16 = ('dis_conv2d_wgrad_bf16x3', 'conv_wgrad_bf16x3_kernel<16|32,16|32>')

# fwd / dgrad: the exact tag of the dis_convg_run call of the forward / the input gradient (dgrad None: the layer has none).  A
# phased call (transposed conv, input gradient of a stride-2 layer) that runs as four parity launches reports the LAST launch's tag:
# class (1, 1), which has the most taps.  wgrad: (entry point, tag).  split3: (fwd, dgrad, wgrad) under conv_split('bf16x3') for the
# cases that also run there, else None.  slot: (ldx, xoff, ldy, yoff, ldg, goff): x is read from, y written into (ops.ConcatBuf slot,
# out=) and gy read from channel ranges of wider buffers whose other lanes hold a fill value.  ref32: the host reference of the GPU
# test is computed with fp32 torch ops on the CPU - legitimate exactly because the bounds < 2^24 are asserted, and checked against
# float64 in the CPU file; these are the 400 000-position slices and the large-tile cases, whose float64 run on a host with few cores
# takes many seconds.  dens: wide values per eligible position (lowered where the weight-gradient bound asks for it, never to zero).
Case = collections.namedtuple('Case', 'id cin_w cin_mem cout k stride transposed h w n crop relu fwd dgrad wgrad split3 slot ref32 '
                                      'dens faults need_dgrad')


def _c(id, cin_w, cin_mem, cout, k, stride, h, w, relu, fwd, dgrad, wgrad, n=2, transposed=False, crop=False, split3=None, slot=None,
       ref32=False, dens=0.1, faults=True, need_dgrad=True):
    return Case(id, cin_w, cin_mem, cout, k, stride, transposed, h, w, n, crop, relu, fwd, dgrad, wgrad, split3, slot, ref32, dens,
                faults, need_dgrad)


CASES = [
    # ---- fp32 MFMA streaming: cin_mem < 32 (CG3_CK), under either split ----
    # tap-packed: cin_mem = 4 and more than 4 taps; no input gradient (the network input); one-pass stem weight gradient with its bias
    _c('f32_stem_k7s2', 2, 4, 32, 7, 2, 20, 18, True, FP32, None, ONE_STEM, need_dgrad=False, split3=(FP32, None, ONE_STEM)),
    _c('f32_16_16', 16, 16, 16, 3, 1, 16, 12, True, FP32, FP32, ONE2_16_16),
    # ragged second 16-chunk (CG_CK): one real channel + 3 padding lanes; pairs k3 s1 with 16 outputs
    _c('f32_17in20_16', 17, 20, 16, 3, 1, 16, 12, False, FP32, FP32, PAIRS2, split3=(FP32, FP32, PAIRS3)),
    # four parity launches on the fp32 kernel: the input gradient of a stride-2 layer with cout < 32 ... (forward: convg2, bn 16;
    # wgrad: k3 s2 pairs need >= 32 gradient channels -> generic)
    _c('f32_dgrad4_32_16_s2', 32, 32, 16, 3, 2, 13, 11, True, G2, FP32, GENERIC),
    # ... and a transposed conv with cin < 32, cropped in both directions (15 x 13 of 16 x 14)
    _c('f32_tconv4_16_16', 16, 16, 16, 3, 2, 8, 7, False, FP32, FP32, GENERIC, transposed=True, crop=True),
    # ---- convg2 streaming: cin >= 32, < 1024 positions per image; cout blocks 16 / 32 / 64 ----
    _c('g2_32_16', 32, 32, 16, 3, 1, 9, 13, False, G2, FP32, ONE2_32_16),
    # the same through channel ranges: x not dense -> no one-pass weight gradient: pairs with 16 outputs; bias with the activation
    _c('g2_32_16_slot', 32, 32, 16, 3, 1, 9, 13, True, G2, FP32, PAIRS2, slot=(40, 4, 24, 8, 20, 4)),
    # bn 32, odd sizes; 25 taps x 2 chunks = 50 k-steps on one workgroup column: already split-K (4 splits of 12 / 13 - cg2_ksplit asks
    # for >= 48 k-steps, not for many channels); the input gradient of a stride-2 layer as four convg2 launches (classes of 9, 6, 6, 4
    # taps x 1 chunk: no split); pairs k5 s2
    _c('g2_k5s2', 64, 64, 32, 5, 2, 21, 19, True, G2_SK, G2, PAIRS2, split3=(G3, G3, PAIRS3)),
    # bn 64, the second block holds 8 channels; bias by dis_colsum (256 % 18 != 0)
    _c('g2_64_72', 64, 64, 72, 3, 1, 9, 13, True, G2, G2, PAIRS2, split3=(G3, G3, PAIRS3)),
    # five 32-channel chunks, the fifth holds one real channel + 3 padding lanes
    _c('g2_129in132_64', 129, 132, 64, 3, 1, 12, 10, False, G2, G2, PAIRS2, split3=(G3, G3, PAIRS3)),
    # 18 positions in all: one ragged tile; image 2 holds narrow values only
    _c('g2_tiny', 64, 64, 32, 3, 1, 3, 2, True, G2, G2, PAIRS2, n=3),
    # 49 taps x 1 chunk = 49 k-steps: split-K again, 4 uneven splits (12, 12, 12, 13), forward and input gradient; pairs k7 s1 (two
    # tap-row groups)
    _c('g2_k7', 32, 32, 32, 7, 1, 13, 11, False, G2_SK, G2_SK, PAIRS2, split3=(G3, G3, PAIRS3)),
    # transposed conv as four convg2 launches, cropped; pairs k3 s2 with x / gy swapped
    _c('g2_tconv_crop', 64, 64, 32, 3, 2, 8, 7, True, G2, G2, PAIRS2, transposed=True, crop=True, split3=(G3, G3, PAIRS3)),
    # ---- convg2 split-K: fewer than 256 workgroups and >= 48 k-steps ----
    _c('sk_512_512', 512, 512, 512, 3, 1, 8, 7, False, G2_SK, G2_SK, PAIRS2),                 # 144 k-steps in 8 splits of 18
    _c('sk_384_64', 384, 384, 64, 3, 1, 8, 7, True, G2_SK, G2, PAIRS2),                       # 108 k-steps in 8 uneven splits (dgrad: 18 k-steps)
    _c('sk_256_128_k5', 256, 256, 128, 5, 1, 6, 5, False, G2_SK, G2_SK, PAIRS2),              # 200 in 8 (dgrad: 100 in 8); pairs k5 s1
    # forward 72 k-steps in 6 splits; input gradient: classes of 1, 2, 2, 4 taps x 32 chunks, the last (128 k-steps) in 8 splits
    _c('sk_dgrad_s2', 256, 256, 1024, 3, 2, 16, 14, True, G2_SK, G2_SK, PAIRS2),
    # ---- convg2 256 x 128 tiles (cg2_big_for: both channel counts >= 128, cout % 128 == 0, workgroups x splits >= 192) ----
    # 8100 positions = 32 tiles of 256, 72 k-steps in 6 splits: 192, the threshold (input gradient 128 -> 256: 36 k-steps, 64 tiles: not big)
    _c('big_sk', 256, 256, 128, 3, 1, 30, 30, True, G2_BIG_SK, G2, PAIRS2, n=9, ref32=True, faults=False),
    # without split-K: 36 k-steps (< 48), so the tiles alone must make 192 workgroups: 49 011 positions = 192 tiles, the smallest
    # n x 31 x 31 that does.  The slowest host reference of the table after the slices: it cannot be smaller and keep the form.
    _c('big_plain', 128, 128, 128, 3, 1, 31, 31, False, G2_BIG, G2_BIG, PAIRS2, n=51, ref32=True, faults=False),
    # ---- convh2 halo: >= 1024 positions per image ----
    # resident weights (NH 8); input gradient from 16 channels: fp32 kernel; one-pass weight gradient
    _c('h2_res_32_16', 32, 32, 16, 3, 1, 40, 36, True, H2_RES, FP32, ONE2_32_16),
    _c('h2_res_32_16_slot', 32, 32, 16, 3, 1, 40, 36, False, H2_RES, FP32, PAIRS2, slot=(36, 4, 20, 4, 24, 8)),
    # streamed weights, 16-row tiles (hv = 33 >= 32; halo 18 x 18: NH 14), 5 weight groups of 2 k-steps
    _c('h2_t16_256_256', 256, 256, 256, 3, 1, 33, 35, True, H2, H2, PAIRS2),
    # streamed weights, 8-row tiles (stride 2: the 33 x 33 halo of 16 rows does not fit; 17 x 33: NH 20), ragged fifth chunk;
    # its input gradient: four phases in ONE launch, streamed weights, 64-wide block (halo 9 x 17: NH 8)
    _c('h2_t8_129in132_s2', 129, 132, 64, 3, 2, 64, 66, False, H2, H2_4PH, PAIRS2),
    # column walk <32, kc 7> (halo 22 x 22: NH 16) and <64, kc 5> (20 x 20: NH 14), ragged tiles
    _c('h2_kc7', 32, 32, 32, 7, 1, 36, 40, False, H2_KC, H2_KC, PAIRS2),
    _c('h2_kc5', 64, 64, 64, 5, 1, 33, 37, True, H2_KC, H2_KC, PAIRS2),
    # four phases in one launch, resident weights: a transposed conv, cropped (65 x 75 of 66 x 76) ...
    _c('h2_tconv4_res', 32, 32, 16, 3, 2, 33, 38, True, H2_4PH_RES, FP32, PAIRS2, transposed=True, crop=True),
    # ... and the input gradient of a stride-2 layer (forward: stride-2 halo, streamed, 8-row tiles)
    _c('h2_dgrad4_res_s2', 32, 32, 32, 3, 2, 66, 64, True, H2, H2_4PH_RES, PAIRS2),
    # four phases in one launch, streamed weights (64-wide block); input gradient: stride-2 halo, streamed
    _c('h2_tconv4_streamed', 128, 128, 64, 3, 2, 35, 32, False, H2_4PH, H2, PAIRS2, transposed=True),
    # four phases refused (streamed, block < 64): one halo launch per phase, each with resident weights; the 1-tap class (0, 0) has an
    # 8 x 16 halo (NH 4), the last, 4-tap class a 9 x 17 one (NH 8)
    _c('h2_tconv_per_phase', 64, 64, 32, 3, 2, 32, 35, True, H2_RES, H2, PAIRS2, transposed=True),
    # (the two-taps-per-k-step halo plan, TP = 2, needs cin <= 16, but the two-term path needs cin >= 32: not reachable by shape on
    #  fp32 storage.  The (64-wide, 64 x 66, stride-2) input gradient of a 64 -> 128 k3 s2 layer at 40 x 36 has 360 positions per
    #  class and streams; h2_t8_129in132_s2 and h2_dgrad4_res_s2 are the halo forms of that input gradient.)
    # ---- 32 x 32 channel slices of conv2d.hip / conv_f16x2.hip: k3 / k7 s1, n h w >= 400 000, <= 10 slice pairs; cin < 32 keeps ----
    # ---- 16 -> 16 off the halo form under either split; fp32 host reference (401 408 positions) ----
    _c('sl_16_16', 16, 16, 16, 3, 1, 448, 448, True, SL2, SL2, ONE2_16_16, ref32=True, dens=0.01, faults=False,
       split3=(SL3, SL3, ONE3_16_16)),
    # ragged slices of 16 input and 8 output channels; two input slices accumulate; bias by dis_colsum (256 % 10 != 0)
    _c('sl_48_40', 48, 48, 40, 3, 1, 448, 448, True, SL2, SL2, PAIRS2, ref32=True, dens=0.01, faults=False),
    # 7 x 7 as seven accumulating tap-row launches: the three-term kernel under either split; 16 gradient channels: generic k7 wgrad
    _c('sl_16_16_k7', 16, 16, 16, 7, 1, 448, 448, False, SL3, SL3, GENERIC, ref32=True, dens=0.01, faults=False),
]
CASE_IDS = [c.id for c in CASES]


def case(case_id):
    return CASES[CASE_IDS.index(case_id)]


def wide_ints(g, shape, lo, hi, eligible, dens, forced=()):
    """float64 tensor of `shape`: dense integers in [lo, hi]; where `eligible` (bool, broadcastable) a fraction `dens` of the entries is
    replaced by +-WIDE, and every index of `forced` is."""
    t = torch.randint(lo, hi + 1, shape, generator=g).double()
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    pick = (torch.rand(shape, generator=g) < dens) & eligible
    for idx in forced:
        pick[idx] = True
    return torch.where(pick, sign * WIDE, t)


def _even(c):
    return (torch.arange(c) % 2 == 0)


def act_eligible(n, c, image):
    """(n, c, 1, 1) mask: image `image`, even channels"""
    return ((torch.arange(n) == image).view(n, 1, 1, 1) & _even(c).view(1, c, 1, 1))


def make_inputs(c):
    """-> x (n, cin_w, h, w), w, b, go (n, cout, oh, ow): float64 integers"""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    oh, ow = out_hw(c)
    ce_in, ce_out = (c.cin_w - 1) // 2 * 2, (c.cout - 1) // 2 * 2               # last even channels
    co_in, co_out = (c.cin_w // 2) * 2 - 1, (c.cout // 2) * 2 - 1               # last odd channels
    x = wide_ints(g, (c.n, c.cin_w, c.h, c.w), -2, 2, act_eligible(c.n, c.cin_w, 0), c.dens, [(0, ce_in, c.h - 1, c.w - 1)])
    odd_o, odd_i = ~_even(c.cout), ~_even(c.cin_w)
    if c.transposed:
        wshape, el = (c.cin_w, c.cout, c.k, c.k), odd_i.view(-1, 1, 1, 1) & odd_o.view(1, -1, 1, 1)
        forced = [(co_in, co_out, 0, 0), (co_in, co_out, c.k - 1, c.k - 1)]
    else:
        wshape, el = (c.cout, c.cin_w, c.k, c.k), odd_o.view(-1, 1, 1, 1) & odd_i.view(1, -1, 1, 1)
        forced = [(co_out, co_in, 0, 0), (co_out, co_in, c.k - 1, c.k - 1)]
    w = wide_ints(g, wshape, -2, 2, el, c.dens, forced)
    b = dense_ints(g, (c.cout,), -8, 8)
    go = wide_ints(g, (c.n, c.cout, oh, ow), -2, 2, act_eligible(c.n, c.cout, 1), c.dens, [(1, ce_out, oh - 1, ow - 1)])
    return x, w, b, go


def run_ref(c, x, w, b, go, dtype=torch.float64):
    """-> y, gx, gw, gb of the layer (+ ReLU when c.relu) in `dtype`"""
    xr, wr, br = [t.to(dtype).clone().requires_grad_(True) for t in (x, w, b)]
    y = conv_op(c, xr, wr, br)
    if c.relu:
        y = F.relu(y)
    y.backward(go.to(dtype))
    return y.detach(), xr.grad, wr.grad, br.grad


def bounds(c, x, w, b, go, dtype=torch.float64):
    """the L1 bounds: max(conv(|x|, |w|) + |b|); max of the input gradient from |go|; max over gw from |x|, |go| and over gb"""
    xa, wa = x.abs().to(dtype).requires_grad_(True), w.abs().to(dtype).requires_grad_(True)
    ya = conv_op(c, xa, wa, b.abs().to(dtype))
    gxa, gwa = torch.autograd.grad(ya, (xa, wa), go.abs().to(dtype))
    gba = go.abs().to(dtype).sum(dim=(0, 2, 3))
    return float(ya.detach().max()), float(gxa.max()), max(float(gwa.max()), float(gba.max()))


Ref = collections.namedtuple('Ref', 'x w b go y gx gw gb y_bound gx_bound gw_bound')


@functools.lru_cache(maxsize=2)
def reference(case_id):
    """inputs, reference results (float64; computed in fp32 for the ref32 cases) and the three L1 bounds of a case (treat as read-only)"""
    c = case(case_id)
    dtype = torch.float32 if c.ref32 else torch.float64
    x, w, b, go = make_inputs(c)
    if c.ref32:
        x, w, b, go = [t.float() for t in (x, w, b, go)]
    y, gx, gw, gb = run_ref(c, x, w, b, go, dtype)
    return Ref(x, w, b, go, y, gx, gw, gb, *bounds(c, x, w, b, go, dtype))


# ---------------------------------------------------------------------------------------------------------------------
# emulation of the two-term fp16 split (tests/test_int_conv_f32_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def split2(v, per_image):
    """v -> (h1, h2) in v's dtype and units: one power-of-two scale s per block (an image of an activation tensor, or the whole weight
    tensor) taking the block's largest magnitude into [2^14, 2^15); h1 = fp16(v s), h2 = fp16(v s - h1), both divided by s again"""
    m = v.abs().amax(dim=tuple(range(1, v.dim())), keepdim=True) if per_image else v.abs().max()
    e = torch.frexp(m.double()).exponent            # m = f 2^e, f in [0.5, 1)
    s = torch.where(m > 0, torch.exp2((15 - e).double()), torch.ones_like(m, dtype=torch.float64)).to(v.dtype)
    vs = v * s
    h1 = vs.half().to(v.dtype)
    h2 = (vs - h1).half().to(v.dtype)
    assert bool(torch.isfinite(h1).all())
    return h1 / s, h2 / s


def op_fwd(c, x, w):
    return conv_op(c, x, w, None)


def op_dgrad(c, g, w):
    """the input gradient: bilinear in (g, w)"""
    xz = torch.zeros((c.n, c.cin_w, c.h, c.w), dtype=g.dtype, requires_grad=True)
    return torch.autograd.grad(conv_op(c, xz, w, None), xz, g)[0]


def op_wgrad(c, x, g):
    """the weight gradient: bilinear in (x, g)"""
    shape = (c.cin_w, c.cout, c.k, c.k) if c.transposed else (c.cout, c.cin_w, c.k, c.k)
    wz = torch.zeros(shape, dtype=x.dtype, requires_grad=True)
    return torch.autograd.grad(conv_op(c, x, wz, None), wz, g)[0]


def emulate(op, c, a, b):
    """the three products of the two-term split of a bilinear op, a = (a1, a2), b = (b1, b2) -> (a1 b1 + a1 b2 + a2 b1, a2 b2)"""
    return op(c, a[0], b[0]) + op(c, a[0], b[1]) + op(c, a[1], b[0]), op(c, a[1], b[1])
