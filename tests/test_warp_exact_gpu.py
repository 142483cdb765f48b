"""The feature warp (csrc/layout_ops.hip: gather_warped_feat forward, atomic backward, the scatter index dis_gather_csr_build and both
index backwards) BIT FOR BIT against float64 on dyadic inputs, and against float64 under derived bars on real-valued ones.

tests/test_net_ops_gpu.py holds these kernels to an independent reference at ONE shape of 1440 destinations (one scan block of the index
build); its larger shapes compare two kernels that read the same index.  Here the inputs are those of tests/warp_ref.py: h - 1 and
w - 1 powers of two, flows multiples of 1/8, integer features and gradients.  Every fp32 step of the kernels is then exact (the
conditions are asserted in warp_ref.dyadic_inputs and again, on the CPU, in tests/test_warp_ref_cpu.py), so the forward output, the
index's offsets and entries, and every backward form must EQUAL the float64 statement: a lost, doubled or misplaced tap is a
difference of at least 1/64.  A failure with differences that are not multiples of 1/64 would mean the exactness argument failed,
not that a tolerance is missing.

The only non-zero bars in this file are the two of test_real_valued_against_fp64, derived where they are asserted."""
import os
import time

import numpy as np
import pytest
import torch

from tests import warp_ref as W

pytestmark = pytest.mark.gpu

GT_TW = 32     # csrc/layout_ops.hip: tile width of the tiled kernels


def _diff(name, got, exp):
    """None if the device tensor equals the float64 reference in every element (torch.equal on the float64 casts), else W.diff's
    message: the count and the first few (index, got, expected)"""
    g, e = got.detach().double().cpu(), torch.tensor(np.asarray(exp), dtype=torch.float64)
    if g.shape == e.shape and torch.equal(g, e):
        return None
    return W.diff(name, g.numpy(), e.numpy())


def _fwd_tiled(tl, c):
    """dis_gather_warped_feat_fwd's dispatch condition, restated: these launches report no kernel tag through lib.profile_start /
    profile_stop (only the conv dispatchers do), so which form serves a shape is DERIVED here, not observed.  The tiled form needs the
    tl * c / 4 threads of a pixel to divide the 256 of a workgroup, and the pixels of a pass to divide the tile width."""
    tpp = tl * (c // 4)
    return tpp <= 256 and 256 % tpp == 0 and GT_TW % (256 // tpp) == 0


def _bwd_tiled(c):
    cg = c // 4
    return cg <= 256 and 256 % cg == 0 and GT_TW % (256 // cg) == 0


def _index_words(csr, tl, bs, h, w, total):
    """the int32 words of the index buffer (layout_ops.hip, above csr_zero_kernel), nd = tl * bs * h * w destinations:
         [0, nd]            offsets (nd + 1 of them; offsets[nd] = number of entries)
         [nd + 1, 2 nd + 1) cursors, scratch of the build
         [2 nd + 1, ...)    entries, two words each: (row of grad_out, bits of the fp32 weight); room for 4 (tl - 1) nd of them
    -> offsets, the first `total` entries as (total, 2)"""
    nd = tl * bs * h * w
    words = csr.cpu().numpy()
    assert words.dtype == np.int32 and words.size >= 2 * nd + 1 + 2 * 4 * (tl - 1) * nd and total <= 4 * (tl - 1) * nd
    return words[:nd + 1], words[2 * nd + 1:2 * nd + 1 + 2 * total].reshape(total, 2)


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).cuda()


def _run_forms(feat, flows, go, init, csr, shape):
    """forward, atomic backward and index backward (without / with init) through the C ABI into NaN-filled outputs, with
    DIS_GATHER_TILED unset (the dispatcher's choice) and set to 0 (the grid-stride kernels) -> {mode: (out, g_atomic, g, g_init)}"""
    from depthinspace_amd import ops
    L = ops.lib
    tl, bs, c, h, w = shape
    assert 'DIS_GATHER_TILED' not in os.environ
    res = {}
    for mode in (None, '0'):
        if mode is not None:
            os.environ['DIS_GATHER_TILED'] = mode
        try:
            out = torch.full((tl, bs, h, w, tl, c), float('nan'), device='cuda')
            L.call('dis_gather_warped_feat_fwd', feat, flows, out, tl, bs, h, w, c)
            ga = torch.full((tl, bs, h, w, c), float('nan'), device='cuda')
            L.call('dis_gather_warped_feat_bwd', go, flows, ga, tl, bs, h, w, c)
            gf = torch.full((tl, bs, h, w, c), float('nan'), device='cuda')
            L.call('dis_gather_warped_feat_bwd_csr', go, csr, None, gf, tl, bs, h, w, c)
            gi = torch.full((tl, bs, h, w, c), float('nan'), device='cuda')
            L.call('dis_gather_warped_feat_bwd_csr', go, csr, init, gi, tl, bs, h, w, c)
            res['tiled unset' if mode is None else 'tiled=0'] = (out, ga, gf, gi)
        finally:
            os.environ.pop('DIS_GATHER_TILED', None)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize('param', W.DYADIC_PARAMS, ids=W.param_id)
def test_warp_equals_fp64_on_dyadic_inputs(param):
    from depthinspace_amd import ops
    shape, case = param
    tl, bs, c, h, w = shape
    r = W.dyadic_reference(shape, case)          # (asserts the conditions on the inputs before any device work)
    st = W.branch_stats(shape, r.offsets)
    # which form the dispatcher takes with DIS_GATHER_TILED unset: derived from the dispatch condition (see _fwd_tiled)
    forms = dict(forward='tiled' if _fwd_tiled(tl, c) else 'grid-stride', index_backward='tiled' if _bwd_tiled(c) else 'grid-stride')
    print(f'{W.param_id(param)}: {forms}, {st}')
    if tl == 3:
        assert forms['forward'] == 'grid-stride'          # 3 * c / 4 threads per pixel never divide 256
    if shape == W.DYADIC_SHAPES[0]:
        assert forms == dict(forward='tiled', index_backward='tiled')
    t0 = time.time()
    feat, flows, go, init = (_dev(a) for a in (r.inp.feat, r.inp.flows, r.inp.go, r.inp.init))
    bad = []
    csr = ops.gather_csr(flows)
    total = int(r.offsets[-1])
    offsets, entries = _index_words(csr, tl, bs, h, w, total)
    bad += W.csr_diff(offsets, entries, r.offsets, r.entries)
    for mode, (out, ga, gf, gi) in _run_forms(feat, flows, go, init, csr, shape).items():
        bad.append(_diff(f'{mode}: forward', out, r.out))
        bad.append(_diff(f'{mode}: atomic backward', ga, r.grad))
        bad.append(_diff(f'{mode}: index backward', gf, r.grad))
        bad.append(_diff(f'{mode}: index backward with init', gi, r.grad_init))
    spent = time.time() - t0
    print(f'{W.param_id(param)}: device part and comparison {spent:.2f} s')
    bad = [b for b in bad if b]
    for b in bad:
        print(f'{W.param_id(param)}: {b}')
    assert not bad, bad
    assert spent < 10.0, spent


@pytest.mark.parametrize('case', W.CASES)
def test_warp_autograd_equals_fp64_on_dyadic_inputs(case):
    """ops.gather_warped_feat as the network calls it, with the index (its backward) and without (the atomic backward)"""
    from depthinspace_amd import ops
    shape = W.DYADIC_SHAPES[0]
    r = W.dyadic_reference(shape, case)
    flows, go = _dev(r.inp.flows), _dev(r.inp.go)
    for name, csr in (('index', ops.gather_csr(flows)), ('atomic', None)):
        feat = _dev(r.inp.feat).requires_grad_(True)
        out = ops.gather_warped_feat(feat, flows, csr)
        out.backward(go)
        msg = _diff(f'{name}: forward', out, r.out) or _diff(f'{name}: gradient', feat.grad, r.grad)
        assert msg is None, msg


def test_index_rebuilt_into_a_used_buffer():
    """dis_gather_csr_build twice into the SAME buffer, first the `converge` flows (long lists, cursors far from zero), then the
    `random` ones: the second index equals the reference for `random` - cursors, block sums and entries of the first build are gone"""
    from depthinspace_amd import lib
    shape = W.DYADIC_SHAPES[0]
    tl, bs, c, h, w = shape
    first, second = W.dyadic_reference(shape, 'converge'), W.dyadic_reference(shape, 'random')
    assert int(first.offsets[-1]) != int(second.offsets[-1])
    buf = torch.empty(lib.fn('dis_gather_csr_workspace')(tl, bs, h, w), dtype=torch.int32, device='cuda')
    for r in (first, second):
        lib.call('dis_gather_csr_build', _dev(r.inp.flows), buf, tl, bs, h, w)
        offsets, entries = _index_words(buf, tl, bs, h, w, int(r.offsets[-1]))
        msgs = W.csr_diff(offsets, entries, r.offsets, r.entries)
        assert not msgs, msgs


@pytest.mark.parametrize('case', ['random', 'converge'])
def test_index_build_repeats(case):
    """two builds from the same flows: the fill order of a list depends on the order the atomics arrive in, the sorted index does not"""
    from depthinspace_amd import ops
    shape = W.DYADIC_SHAPES[0]
    tl, bs, c, h, w = shape
    r = W.dyadic_reference(shape, case)
    flows = _dev(r.inp.flows)
    a, b = ops.gather_csr(flows), ops.gather_csr(flows)
    nd = tl * bs * h * w
    total = int(a[nd])
    assert total == int(b[nd]) == int(r.offsets[-1])
    assert torch.equal(a[:nd + 1], b[:nd + 1])
    assert torch.equal(a[2 * nd + 1:2 * nd + 1 + 2 * total], b[2 * nd + 1:2 * nd + 1 + 2 * total])


# ---------------------------------------------------------------------------------------------------------------------
# real-valued inputs at sizes that are not 2^k + 1
# ---------------------------------------------------------------------------------------------------------------------
REAL_SHAPES = [(4, 2, 32, 37, 45), (3, 2, 32, 24, 200), (2, 3, 64, 21, 8), (4, 1, 16, 130, 70)]
EPS = 2.0 ** -24     # unit roundoff of fp32


@pytest.mark.parametrize('tl,bs,c,h,w', REAL_SHAPES)
def test_real_valued_against_fp64(tl, bs, c, h, w):
    """N(0,1) features and gradients, flows 5 N(0,1): forward, atomic backward and index backward, dispatcher's choice and grid-stride,
    against the float64 statement.  The bars are derived, not tuned:

    position.  flow + pixel and the four operations of the normalisation round trip are at most 5 fp32 roundings of values of
      magnitude up to the image size: |d position| <= 5 EPS max(h, w) per axis (positions far outside have no valid tap in either).
    forward.  A bilinear surface (zeros outside) changes by at most 2 max|feat| per unit of position along an axis (neighbouring
      samples differ by at most that); two axes: 2 * 2 max|feat| * 5 EPS max(h, w); plus the 4-term fp32 sum of products, each
      bounded by max|feat|:
          |out - ref| <= (20 max(h, w) + 4) EPS max|feat|
    backward.  Each entry's weight is off by at most 20 max(h, w) EPS (the same Lipschitz argument on the weight, which is continuous
      across the integer positions where a tap appears with weight 0); a destination sums at most `longest` entries (the longest list
      of the float64 index) of gradients up to max|go|; the fp32 accumulation adds `longest` roundings of partial sums no larger than
      S = max over destinations and channels of |go slot 0| + sum w |go row| (the float64 backward of |go|):
          |grad - ref| <= longest (20 max(h, w) EPS max|go| + EPS S)"""
    from depthinspace_amd import ops
    g = torch.Generator().manual_seed(tl * 100 + c + h)
    feat = torch.randn(tl, bs, h, w, c, generator=g)
    flows = torch.randn(tl * tl, bs, h, w, 2, generator=g) * 5
    go = torch.randn(tl, bs, h, w, tl, c, generator=g)
    ref_out = W.forward(feat.numpy(), flows.numpy())
    ref_grad = W.backward(go.numpy(), flows.numpy())
    longest = int(W.list_lengths(W.csr(flows.numpy())[0]).max())
    S = float(W.backward(go.abs().numpy(), flows.numpy()).max())
    bar_f = (20 * max(h, w) + 4) * EPS * float(feat.abs().max())
    bar_b = longest * (20 * max(h, w) * EPS * float(go.abs().max()) + EPS * S)
    fd, fl, god = feat.cuda(), flows.cuda(), go.cuda()
    res = _run_forms(fd, fl, god, torch.zeros(tl, bs, h, w, c, device='cuda'), ops.gather_csr(fl), (tl, bs, c, h, w))
    worst = []
    for mode, (out, ga, gf, gi) in res.items():
        e_f = float((out.double().cpu() - torch.from_numpy(ref_out)).abs().max())
        errs = [float((t.double().cpu() - torch.from_numpy(ref_grad)).abs().max()) for t in (ga, gf, gi)]
        print(f'tl{tl}_bs{bs}_c{c}_{h}x{w} {mode}: forward {e_f:.3e} (bar {bar_f:.3e}); atomic backward {errs[0]:.3e}, index backward '
              f'{errs[1]:.3e}, with a zero init {errs[2]:.3e} (bar {bar_b:.3e}; longest list {longest}, S {S:.2f})')
        worst.append((e_f, max(errs)))
    for e_f, e_b in worst:
        assert e_f <= bar_f       # NaN (an element never written) fails both
        assert e_b <= bar_b
