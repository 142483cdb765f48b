"""float64 numpy statement of the feature warp (gather_warped_feat, csrc/layout_ops.hip) and of the scatter index its backward uses,
with inputs on which fp32 arithmetic is EXACT.  No torch, no GPU.

The operation (reference model/multi_frame_networks.py:347-360, warp :83-99; oracle.dis_oracle._gather_warped_feat):
    feat  (tl, bs, h, w, c)       flows (tl * tl, bs, h, w, 2): flows[t * tl + j] = the flow (x, y) from target t into frame j
    out   (tl, bs, h, w, tl, c):  out[t, :, :, :, 0] = feat[t]; slot s >= 1 holds frame j = the s-th of the OTHER frames in increasing
                                  order, sampled bilinearly (zeros outside the image) at pixel + flows[t * tl + j]
The sample position goes through the reference's normalisation and back, (2 (p / (size - 1) - 1/2) + 1) (size - 1) / 2, and is then
clamped to [-2, size + 2]: every position outside (-1, size) has no tap inside the image, so the clamp changes no result, it only keeps
the integer conversion of far-out positions (sentinel flows) defined.

Backward: grad_feat[j, b, q] = grad_out[j, b, q, slot 0] (+ init) + sum over the taps that landed on (j, b, q) of weight * grad_out[row].
The scatter index lists those taps per DESTINATION d = (j * bs + b) * h * w + q: (row of grad_out viewed as (tl * bs * h * w * tl, c),
weight), one entry per VALID tap - a tap inside the image whose weight is zero is listed too - sorted by row.  A row (t, b, p, s) reaches
four different destinations, so rows are unique within a list and the sorted index is fully determined.

Exactness (dyadic_inputs): with h - 1 and w - 1 powers of two and flows that are multiples of 1/8, every step of taps() is exact in
fp32 - the division by size - 1, the floor, the four weight products (multiples of 1/64); with integer features and gradients every
product and partial sum is a small multiple of 1/64, far below 2^24 in any order.  So forward, index and every backward form must EQUAL
what is computed here, and a lost, doubled or misplaced tap is a difference of at least 1/64."""
import collections
import functools

import numpy as np

Taps = collections.namedtuple('Taps', 'x0 y0 w v')    # w, v: (4, ...) in the order (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1)
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))            # (dy, dx)
SENTINEL = np.float32(1e30)


def shape_of(flows):
    t2, bs, h, w, two = flows.shape
    tl = int(round(t2 ** 0.5))
    assert tl * tl == t2 and two == 2 and tl >= 2, flows.shape
    return tl, bs, h, w


def others(t, tl):
    """the frames held by slots 1 .. tl - 1 of target t"""
    return [j for j in range(tl) if j != t]


def taps(flows, h, w, dtype=np.float64):
    """flows (..., h, w, 2) -> Taps of arrays shaped (..., h, w), every step carried out in `dtype`"""
    T = dtype
    f = np.asarray(flows).astype(T)
    assert f.shape[-3:] == (h, w, 2), f.shape

    def position(p, size):
        g = T(2) * (p / T(size - 1) - T(0.5))
        i = (g + T(1)) * (T(size - 1) / T(2))
        assert i.dtype == T
        return np.clip(i, T(-2), T(size + 2))
    ix = position(f[..., 0] + np.arange(w, dtype=T), w)
    iy = position(f[..., 1] + np.arange(h, dtype=T)[:, None], h)
    fx, fy = np.floor(ix), np.floor(iy)
    wx, wy = ix - fx, iy - fy
    ex, ey = T(1) - wx, T(1) - wy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    wgt = np.stack([ey * ex, ey * wx, wy * ex, wy * wx])
    assert wgt.dtype == T
    xin = [(x0 + dx >= 0) & (x0 + dx < w) for dx in (0, 1)]
    yin = [(y0 + dy >= 0) & (y0 + dy < h) for dy in (0, 1)]
    return Taps(x0, y0, wgt, np.stack([yin[dy] & xin[dx] for dy, dx in CORNERS]))


def taps_equal(a, b):
    return bool(np.array_equal(a.x0, b.x0) and np.array_equal(a.y0, b.y0) and np.array_equal(a.v, b.v) and
                np.array_equal(a.w.astype(np.float64), b.w.astype(np.float64)))


def _all_taps(flows, dtype=np.float64):
    tl, bs, h, w = shape_of(flows)
    return taps(np.asarray(flows).reshape(tl, tl, bs, h, w, 2), h, w, dtype)


def forward(feat, flows):
    """-> (tl, bs, h, w, tl, c) float64"""
    tl, bs, h, w = shape_of(flows)
    feat = np.asarray(feat, dtype=np.float64)
    assert feat.shape[:4] == (tl, bs, h, w), feat.shape
    T = _all_taps(flows)
    out = np.zeros((tl, bs, h, w, tl, feat.shape[-1]))
    bi = np.arange(bs)[:, None, None]
    for t in range(tl):
        out[t, :, :, :, 0] = feat[t]
        for s, j in enumerate(others(t, tl), 1):
            for k, (dy, dx) in enumerate(CORNERS):
                yy = np.clip(T.y0[t, j] + dy, 0, h - 1)      # (an invalid tap: any address, weight 0 - zeros padding)
                xx = np.clip(T.x0[t, j] + dx, 0, w - 1)
                wk = np.where(T.v[k, t, j], T.w[k, t, j], 0.0)
                out[t, :, :, :, s] += wk[..., None] * feat[j][bi, yy, xx]
    return out


def tap_list(flows):
    """every valid tap, in no particular order -> (dest, row, weight float64), one element per tap"""
    tl, bs, h, w = shape_of(flows)
    T = _all_taps(flows)
    hw = h * w
    pix = np.arange(hw).reshape(h, w)
    b = np.arange(bs)[:, None, None]
    dest, row, wgt = [], [], []
    for t in range(tl):
        for s, j in enumerate(others(t, tl), 1):
            r = ((t * bs + b) * hw + pix) * tl + s                     # (bs, h, w)
            for k, (dy, dx) in enumerate(CORNERS):
                v = T.v[k, t, j]
                d = (j * bs + b) * hw + (T.y0[t, j] + dy) * w + T.x0[t, j] + dx
                dest.append(d[v])
                row.append(r[v])
                wgt.append(T.w[k, t, j][v])
    return np.concatenate(dest), np.concatenate(row), np.concatenate(wgt)


def csr(flows):
    """-> offsets (nd + 1,) int32, entries (total, 2) int32: (row, bits of the fp32 weight), each destination's list sorted by row"""
    tl, bs, h, w = shape_of(flows)
    nd = tl * bs * h * w
    dest, row, wgt = tap_list(flows)
    order = np.lexsort((row, dest))
    offsets = np.zeros(nd + 1, dtype=np.int64)
    np.cumsum(np.bincount(dest, minlength=nd), out=offsets[1:])
    assert offsets[-1] == dest.size < 2 ** 31 and nd * tl < 2 ** 31
    entries = np.stack([row[order].astype(np.int32), wgt[order].astype(np.float32).view(np.int32)], 1)
    return offsets.astype(np.int32), entries


def backward(go, flows, init=None):
    """go (tl, bs, h, w, tl, c) -> (tl, bs, h, w, c) float64: slot 0 of go, plus init, plus the weighted scatter of the warped slots"""
    tl, bs, h, w = shape_of(flows)
    go = np.asarray(go, dtype=np.float64)
    c = go.shape[-1]
    assert go.shape == (tl, bs, h, w, tl, c), go.shape
    out = go[:, :, :, :, 0].copy()
    if init is not None:
        out += np.asarray(init, dtype=np.float64)
    dest, row, wgt = tap_list(flows)
    flat = out.reshape(-1, c)
    np.add.at(flat, dest, wgt[:, None] * go.reshape(-1, c)[row])
    return flat.reshape(tl, bs, h, w, c)


def list_lengths(offsets):
    return np.diff(np.asarray(offsets, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# comparison helpers of the device tests (numpy in, message out: exercised without a device by tests/test_warp_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def diff(name, got, exp):
    """None if got == exp in every element, else a message with the count and the first few (index, got, expected)"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return f'{name}: shape {got.shape} != {exp.shape}'
    if np.array_equal(got, exp):
        return None
    ne = got != exp            # (NaN != anything: an element the kernel never wrote counts)
    bad = np.argwhere(ne)
    first = [(tuple(int(v) for v in i), got[tuple(i)].item(), exp[tuple(i)].item()) for i in bad[:6]]
    return f'{name}: {bad.shape[0]} of {exp.size} differ; first (index, got, expected): {first}'


def csr_diff(got_offsets, got_entries, ref_offsets, ref_entries):
    """the index the device built against csr(): list of messages, empty if offsets (all nd + 1, so the total too), rows and weight
    bits are equal.  got_entries: at least `total` (row, weight bits) pairs, read up to the REFERENCE's total."""
    msgs = [diff('csr offsets', got_offsets, ref_offsets)]
    total = int(ref_offsets[-1])
    if int(got_offsets[-1]) != total:
        msgs.append(f'csr total: offsets[nd] = {int(got_offsets[-1])}, expected {total}')
    got_entries = np.asarray(got_entries)
    if got_entries.shape[0] < total:
        msgs.append(f'csr entries: room for {got_entries.shape[0]} entries, expected {total}')
    else:
        msgs.append(diff('csr entry rows', got_entries[:total, 0], ref_entries[:, 0]))
        msgs.append(diff('csr entry weight bits', got_entries[:total, 1], ref_entries[:, 1]))
    return [m for m in msgs if m]


# ---------------------------------------------------------------------------------------------------------------------
# dyadic inputs
# ---------------------------------------------------------------------------------------------------------------------
CASES = ('random', 'converge', 'borders', 'ramp')
# (tl, bs, c, h, w): 9 scan blocks of the index build with a ragged last one and ragged 8 x 32 tiles; 66 scan blocks (two block sums
# per lane of the middle scan pass, lanes 33 .. 63 idle); three frames (no tiled forward: 3 * 32 / 4 = 24 does not divide 256); smaller
# than one tile with 64 channels; the smallest map whose h - 1 and w - 1 are powers of two
DYADIC_SHAPES = ((4, 2, 32, 33, 65), (4, 2, 16, 129, 129), (3, 2, 32, 17, 129), (2, 3, 64, 9, 5), (2, 1, 16, 3, 3))
BIG = (4, 2, 16, 129, 129)
SCAN_ELEMS = 2048      # csrc/layout_ops.hip: CSR_SCAN_ELEMS
SORT_MAX = 16          # CSR_SORT_MAX: longer lists take the in-memory insertion sort
FETCH = 12             # GC_E: entries the tiled backward fetches together


def dyadic_cases(shape):
    return ('random',) if tuple(shape) == BIG else CASES


DYADIC_PARAMS = tuple((s, k) for s in DYADIC_SHAPES for k in dyadic_cases(s))


def param_id(p):
    (tl, bs, c, h, w), case = p
    return f'tl{tl}_bs{bs}_c{c}_{h}x{w}_{case}'


def _eighths(rng, shape, lim=8):
    return (rng.integers(-8 * lim, 8 * lim + 1, size=shape) / 8.0).astype(np.float32)


def ramp_layout(tl, h, w):
    """the hand-built destinations of the `ramp` case (frame 0 of every sample) -> {(y, x): list length}; empty on maps too small to
    hold them.  base = 4 (tl - 1): at zero flow every frame's pixel p lands ON p with weight 1 and lists p + 1 in x, in y and in both
    with weight 0, so an interior destination is listed by four pixels of each other frame."""
    if h < 9 or w < 17:
        return {}
    base = 4 * (tl - 1)
    return {(3, 3): 2 * base, (4, 4): 2 * base + 1, (4, 12): base - 1, (7, 9): base + 1, (7, 12): base - 1, (7, 2): base}


def _flows(case, rng, tl, bs, h, w):
    fl = np.zeros((tl, tl, bs, h, w, 2), dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    if case == 'random':
        fl[:] = _eighths(rng, fl.shape)
    elif case == 'converge':
        # every pair (t, j): a block of up to 9 x 9 pixels of t lands on ONE pixel of j (integer flows: weight 1, and the three
        # neighbours listed with weight 0), so that pixel's list holds (tl - 1) * 81 entries and more; the last frame's flows all leave
        # the image: none of its taps is valid, and no list holds a row of it
        fl[:] = _eighths(rng, fl.shape)
        bh, bw = min(9, h), min(9, w)
        for t in range(tl):
            for j in others(t, tl):
                by, bx = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
                ty, tx = (3 * j + 1) % (h - 1), (5 * j + 2) % (w - 1)        # (not the last row / column: all four taps valid)
                fl[t, j, :, by:by + bh, bx:bx + bw, 0] = (tx - xs)[by:by + bh, bx:bx + bw]
                fl[t, j, :, by:by + bh, bx:bx + bw, 1] = (ty - ys)[by:by + bh, bx:bx + bw]
        fl[tl - 1] = 1000.0
    elif case == 'borders':
        # every third row: x positions exactly -1 (one column inside, weight 0), -1/2, 0, w - 1 (weight 1, the neighbour outside),
        # w - 1/2, w (nothing inside); every third column: the same in y; where they cross, both - corners with one valid tap.
        # A patch of sentinel flows of either sign for the clamp.
        fl[:] = _eighths(rng, fl.shape)
        px = np.array([-1, -0.5, 0, w - 1, w - 0.5, w])[(xs + ys // 3) % 6]
        py = np.array([-1, -0.5, 0, h - 1, h - 0.5, h])[(ys + xs // 3) % 6]
        fl[..., 0] = np.where(ys % 3 == 0, px - xs, fl[..., 0])
        fl[..., 1] = np.where(xs % 3 == 0, py - ys, fl[..., 1])
        y1, x1 = min(1, h - 2), min(1, w - 2)
        fl[..., y1, x1, :] = (SENTINEL, -SENTINEL)
        fl[..., y1, x1 + 1, :] = (-SENTINEL, 0.0)
        fl[..., y1 + 1, x1, :] = (0.25, SENTINEL)
        fl[..., y1 + 1, x1 + 1, :] = (-SENTINEL, -SENTINEL)
    elif case == 'ramp':
        # zero flow, and integer shifts INTO frame 0 (see ramp_layout):
        #   rows 2 .. 5, columns 2 .. 9 of every other frame: x shift -ceil((x - 2) / 2), two pixels land on each of the columns 2 .. 5
        #     -> destinations whose 2 x 2 window lies in rows 2 .. 5, columns 2 .. 5 are listed twice by every frame: 2 base
        #   frame 1 only: pixel (4, 12) lands on (4, 4): 2 base + 1 there, base - 1 at (4, 12); pixel (7, 12) lands on (7, 9):
        #     base + 1 there, base - 1 at (7, 12)
        if ramp_layout(tl, h, w):
            for t in range(1, tl):
                fl[t, 0, :, 2:6, 2:10, 0] = -np.ceil((xs[2:6, 2:10] - 2) / 2.0)
            fl[1, 0, :, 4, 12, 0] = -8.0
            fl[1, 0, :, 7, 12, 0] = -3.0
    else:
        raise ValueError(case)
    return fl.reshape(tl * tl, bs, h, w, 2)


Dyadic = collections.namedtuple('Dyadic', 'feat flows go init max_len')


def _pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def dyadic_inputs(case, tl, bs, c, h, w, seed=0):
    """float32 arrays feat (integers in [-8, 8]), flows (multiples of 1/8, and sentinels), go and init (integers in [-4, 4]) and the
    longest list of the index; the conditions under which fp32 arithmetic on them is exact are asserted here, before any device work"""
    assert _pow2(h - 1) and _pow2(w - 1), (h, w)
    rng = np.random.default_rng([seed, CASES.index(case), tl, bs, c, h, w])
    flows = _flows(case, rng, tl, bs, h, w)
    assert flows.dtype == np.float32 and np.isfinite(flows).all()
    f8 = flows.astype(np.float64) * 8
    assert np.array_equal(f8, np.round(f8))
    assert (np.abs(flows[np.abs(flows) < SENTINEL]) <= 1024).all()          # position = flow + pixel: a multiple of 1/8 below 2^11
    assert taps_equal(taps(flows, h, w, np.float32), taps(flows, h, w, np.float64))
    feat = rng.integers(-8, 9, size=(tl, bs, h, w, c)).astype(np.float32)
    go = rng.integers(-4, 5, size=(tl, bs, h, w, tl, c)).astype(np.float32)
    init = rng.integers(-4, 5, size=(tl, bs, h, w, c)).astype(np.float32)
    offsets, _ = csr(flows)
    lens = list_lengths(offsets)
    max_len = int(lens.max())
    # in units of 1/64: |go| <= 4, weights <= 64, max_len entries + slot 0 + init
    assert 64 * 4 * (max_len + 2) < 2 ** 24, max_len
    if case == 'ramp':
        lens0 = lens.reshape(tl, bs, h, w)[0]
        for (y, x), n in ramp_layout(tl, h, w).items():
            assert (lens0[:, y, x] == n).all(), ((y, x), n, lens0[:, y, x])
    return Dyadic(feat, flows, go, init, max_len)


Reference = collections.namedtuple('Reference', 'inp out offsets entries grad grad_init')


@functools.lru_cache(maxsize=None)
def dyadic_reference(shape, case):
    """inputs and float64 results of one (shape, case), computed once per process; treat as read-only"""
    inp = dyadic_inputs(case, *shape)
    offsets, entries = csr(inp.flows)
    grad = backward(inp.go, inp.flows)
    ref = Reference(inp, forward(inp.feat, inp.flows), offsets, entries, grad, grad + inp.init.astype(np.float64))
    for a in (*inp[:4], *ref[1:]):
        a.setflags(write=False)
    return ref


def branch_stats(shape, offsets):
    """what a (shape, flows) reaches: scan blocks of the build, longest list, share of lists beyond the register sort, empty lists"""
    lens = list_lengths(offsets)
    return dict(scan_blocks=-(-lens.size // SCAN_ELEMS), longest=int(lens.max()), over_sort=float((lens > SORT_MAX).mean()),
                empty=float((lens == 0).mean()), at_fetch=[int((lens == n).sum()) for n in (FETCH - 1, FETCH, FETCH + 1)])
