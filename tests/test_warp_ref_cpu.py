"""CPU: tests/warp_ref.py, the float64 statement and the dyadic inputs of tests/test_warp_exact_gpu.py.  The statement against the
oracle's warp and its autograd gradient on real-valued inputs; its two formulations of the backward (scatter over the taps, gather
over the index) against each other, exactly; the conditions that make the device comparison an equality, for every (shape, case) the
device test runs; and the comparison helpers of the device test on an index with one entry removed / one offset moved."""
import numpy as np
import pytest
import torch

from tests import warp_ref as W


def _relerr(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize('tl,bs,c,h,w', [(4, 2, 32, 12, 15), (3, 2, 8, 7, 10)])
def test_forward_and_backward_match_the_oracle(tl, bs, c, h, w):
    """the bars of tests/test_net_ops_gpu.py::test_gather_warped_feat (the oracle runs in fp32): 2e-6 / 1e-5 of the largest entry"""
    from oracle import dis_oracle as O
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(tl, bs, c, h, w, generator=g)
    flow = {f'flow_{i}{j}': torch.randn(bs, 2, h, w, generator=g) * 3 for i in range(tl) for j in range(tl) if i != j}
    fr = feat.clone().requires_grad_(True)
    ref = torch.stack([O._gather_warped_feat(fr, flow, t, tl) for t in range(tl)], 0)       # (tl, slot, bs, c, h, w)
    go = torch.randn(ref.shape, generator=g)
    ref.backward(go)
    flows = np.zeros((tl * tl, bs, h, w, 2), dtype=np.float32)
    for i in range(tl):
        for j in range(tl):
            if i != j:
                flows[i * tl + j] = flow[f'flow_{i}{j}'].permute(0, 2, 3, 1).numpy()
    out = W.forward(feat.permute(0, 1, 3, 4, 2).numpy(), flows)                              # (tl, bs, h, w, slot, c)
    grad = W.backward(go.permute(0, 2, 4, 5, 1, 3).numpy(), flows)                          # (tl, bs, h, w, c)
    e_out = _relerr(out.transpose(0, 4, 1, 5, 2, 3), ref.detach().double().numpy())
    e_grad = _relerr(grad.transpose(0, 1, 4, 2, 3), fr.grad.double().numpy())
    print(f'forward {e_out:.2e}, backward {e_grad:.2e}')
    assert e_out < 2e-6
    assert e_grad < 1e-5
    # (the comparison is not one of zeros, and some taps leave the image)
    assert float(ref.detach().abs().max()) > 1 and not W.taps(flows, h, w).v.all()


def _backward_from_index(go, offsets, entries, init):
    """the gather formulation: per destination, slot 0 + init + the sum over its list (a difference of running sums: exact in float64
    on dyadic data, whose running sums are multiples of 1/64 far below 2^53)"""
    c = go.shape[-1]
    rows = go.reshape(-1, c).astype(np.float64)
    terms = entries[:, 1].copy().view(np.float32).astype(np.float64)[:, None] * rows[entries[:, 0]]
    run = np.concatenate([np.zeros((1, c)), np.cumsum(terms, 0)])
    off = offsets.astype(np.int64)
    out = go[:, :, :, :, 0].astype(np.float64) + init + (run[off[1:]] - run[off[:-1]]).reshape(init.shape)
    return out


@pytest.mark.parametrize('param', W.DYADIC_PARAMS, ids=W.param_id)
def test_dyadic_case_is_exact_and_consistent(param):
    """dyadic_inputs asserts the preconditions (sizes, multiples of 1/8, fp32 taps == fp64 taps, the 2^24 bound, the hand-built list
    lengths); here also: the two backward formulations agree EXACTLY, the index is well formed, every result is a multiple of 1/64
    that fp32 holds, and the case reaches what it is listed for."""
    shape, case = param
    tl, bs, c, h, w = shape
    r = W.dyadic_reference(shape, case)
    inp = r.inp
    nd = tl * bs * h * w
    lens = W.list_lengths(r.offsets)
    assert r.offsets.shape == (nd + 1,) and r.offsets[0] == 0 and (lens >= 0).all() and r.offsets[-1] == r.entries.shape[0]
    assert inp.max_len == lens.max()
    # sorted by row, rows unique within a list: the row sequence increases strictly except where a new list starts
    starts = np.zeros(r.entries.shape[0] + 1, dtype=bool)
    starts[r.offsets.astype(np.int64)] = True
    assert (np.diff(r.entries[:, 0].astype(np.int64)) > 0)[~starts[1:-1]].all()
    wgt = r.entries[:, 1].copy().view(np.float32).astype(np.float64)
    assert np.array_equal(wgt * 64, np.round(wgt * 64)) and ((wgt >= 0) & (wgt <= 1)).all()
    assert np.array_equal(_backward_from_index(inp.go, r.offsets, r.entries, inp.init.astype(np.float64)), r.grad_init)
    for a in (r.out, r.grad, r.grad_init):
        assert np.array_equal(a * 64, np.round(a * 64)) and np.abs(a).max() * 64 < 2 ** 24
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    st = W.branch_stats(shape, r.offsets)
    print(W.param_id(param), st, 'zero-weight entries', int((wgt == 0).sum()))
    if case == 'random' and h * w >= 17 * 129:
        assert st['over_sort'] > (0.01 if tl == 4 else 0)          # (three frames: an interior list holds 8, not 12)
        assert st['over_sort'] < 1 and st['empty'] > 0 and min(st['at_fetch']) > 0
    if case == 'converge':
        bh, bw = min(9, h), min(9, w)
        assert st['longest'] >= (tl - 1) * bh * bw           # (the last frame's pixel: a block of every other frame)
        if (h, w) == (33, 65):
            assert st['longest'] >= 243 and st['longest'] % W.FETCH != 0
        # the last frame's taps all leave the image: no list holds a row of it
        assert (r.entries[:, 0] // tl // (h * w) // bs < tl - 1).all()
        if tl == 2:
            assert (lens[:bs * h * w] == 0).all()
    if shape == (2, 1, 16, 3, 3) and case == 'random':
        assert r.entries.shape[0] == 0                       # (flows up to 8 on a 3 x 3 map: every tap leaves it - an EMPTY index)
    if case == 'borders' and h * w > 9:
        T = W.taps(inp.flows, h, w)
        nvalid = T.v.sum(0)
        assert all((nvalid == n).any() for n in (0, 1, 2, 4))
        assert (wgt == 0).any() and (wgt == 1).any() and (wgt == 0.5).any()
        assert (T.x0 == -2).any() and (T.x0 == w + 2).any() and (T.y0 == -2).any() and (T.y0 == h + 2).any()   # the clamp
    if case == 'ramp' and W.ramp_layout(tl, h, w):
        base = 4 * (tl - 1)
        assert sorted(set(W.ramp_layout(tl, h, w).values())) == [base - 1, base, base + 1, 2 * base, 2 * base + 1]
    if shape == W.DYADIC_SHAPES[0]:
        assert st['scan_blocks'] == 9 and nd % W.SCAN_ELEMS != 0
    if shape == W.BIG:
        assert st['scan_blocks'] == 66


def test_helpers_see_one_lost_entry_and_one_moved_offset():
    """the comparison the device test makes, on the reference itself with one fault: nothing here touches a kernel"""
    shape, case = W.DYADIC_SHAPES[0], 'random'
    r = W.dyadic_reference(shape, case)
    assert W.csr_diff(r.offsets, r.entries, r.offsets, r.entries) == []
    assert W.diff('grad', r.grad.astype(np.float32).astype(np.float64), r.grad) is None
    wgt = r.entries[:, 1].copy().view(np.float32)
    small = np.flatnonzero(wgt == np.float32(1 / 64))
    assert small.size > 0
    e = int(small[small.size // 2])
    d = int(np.searchsorted(r.offsets, e, side='right') - 1)             # the destination whose list holds entry e
    # one entry of weight 1/64 lost: the index differs (offsets and entries), and so does the gradient computed from it
    off2 = r.offsets.copy()
    off2[d + 1:] -= 1
    ent2 = np.delete(r.entries, e, axis=0)
    msgs = W.csr_diff(off2, np.concatenate([ent2, ent2[-1:]]), r.offsets, r.entries)
    assert any('offsets' in m for m in msgs) and any('total' in m for m in msgs) and any('rows' in m for m in msgs), msgs
    g2 = _backward_from_index(r.inp.go, off2, ent2, r.inp.init.astype(np.float64))
    lost = np.abs(g2 - r.grad_init)
    gone = r.inp.go.reshape(-1, shape[2])[r.entries[e, 0]]
    assert np.array_equal(lost.reshape(-1, shape[2])[d], np.abs(gone) / 64) and np.count_nonzero(lost) == np.count_nonzero(gone) > 0
    msg = W.diff('grad', g2, r.grad_init)
    assert msg is not None and f'{np.count_nonzero(gone)} of' in msg
    # one offset moved by one: the entries are the same, the offsets are not
    off3 = r.offsets.copy()
    off3[d + 1] += 1
    msgs = W.csr_diff(off3, r.entries, r.offsets, r.entries)
    assert len(msgs) == 1 and msgs[0].startswith('csr offsets: 1 of'), msgs
    assert not np.array_equal(_backward_from_index(r.inp.go, off3, r.entries, r.inp.init.astype(np.float64)), r.grad_init) or \
        not r.inp.go.reshape(-1, shape[2])[r.entries[r.offsets[d + 1], 0]].any()
    # a weight one unit in the last place off, a NaN left unwritten
    ent4 = r.entries.copy()
    ent4[e, 1] += 1
    assert [m.split(':')[0] for m in W.csr_diff(r.offsets, ent4, r.offsets, r.entries)] == ['csr entry weight bits']
    out = r.out.copy()
    out[-1, -1, -1, -1, -1, -1] = np.nan
    assert '1 of' in W.diff('out', out, r.out)
