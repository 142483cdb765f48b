"""CPU: tests/int_conv_ref.py, the operands and float64 reference of tests/test_convb_exact_gpu.py.  For every row of the GPU case
table: the L1 bounds that make a bit-for-bit comparison legitimate hold, the results survive the bf16 round trip, the float64
reference equals a plain fp32 run of the same torch ops (integers are exact in both), and the faults the method is meant to catch
- a dropped tap, a dropped channel, a shifted transposed-conv phase, a lost pixel row - do change the reference."""
import pytest
import torch

from tests import int_conv_ref as R

BF = torch.bfloat16


def _case(cid):
    return R.CASES[R.CASE_IDS.index(cid)]


def test_table_is_well_formed():
    assert len(set(R.CASE_IDS)) == len(R.CASES)
    relu = sum(1 for c in R.CASES if c.relu)
    assert abs(2 * relu - len(R.CASES)) <= 4, relu          # about half ReLU, half ACT_NONE (the gpre = gy shortcut)
    for c in R.CASES:
        assert c.cin_mem >= c.cin_w and c.cin_mem % (4 if c.x_fp32 else 8) == 0 and c.cout % 8 == 0, c.id
        m = R.m_of(c.cin_w, c.k)
        assert c.k * c.k * m * 2 * 2 + 8 <= R.BOUND, c.id
    tags = {c.fwd for c in R.CASES} | {c.dgrad for c in R.CASES} | {c.wgrad for c in R.CASES}
    for t in (R.STREAM, R.ST128, R.SPLITK, R.BIG, R.HALO, R.HALO_KC, R.HALO_4PH, R.PAIRS, R.WGRAD_GENERIC):
        assert t in tags, t


def test_generators():
    g = torch.Generator().manual_seed(1)
    x = R.sparse_ints(g, 2, 17, 5, 7, 6, c_mem=24)
    assert tuple(x.shape) == (2, 24, 5, 7) and x.dtype == torch.float64
    assert bool(((x != 0).sum(1) == 6).all())                 # exactly m channels per pixel ...
    assert float(x[:, 17:].abs().max()) == 0.0                # ... among the real ones
    assert set(x.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert bool((x[:, :17] != 0).flatten(2).any(2).all())           # every real channel meets nonzero data somewhere
    w = R.dense_ints(g, (4, 3, 3, 3), -2, 2)
    assert set(w.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    b = R.dense_ints(g, (400,), -8, 8)
    assert float(b.min()) == -8 and float(b.max()) == 8 and bool((b == b.round()).all())
    assert [R.m_of(64, k) for k in (3, 5, 7)] == [6, 2, 1] and R.m_of(2, 7) == 1 and R.m_of(1, 3) == 1 and R.m_of(2, 3) == 2


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_case_is_exact_in_bf16_and_fp32(cid):
    c, r = _case(cid), R.reference(cid)
    assert r.y_bound <= R.BOUND and r.gx_bound <= R.BOUND, (r.y_bound, r.gx_bound)
    for t in (r.y, r.gx):
        assert float(t.abs().max()) <= R.BOUND
        assert torch.equal(t.float().to(BF).double(), t)       # the bf16 round trip is exact
    for t in (r.gw, r.gb):
        assert torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24
    y32, gx32, gw32, gb32 = R.run_ref(c, r.x, r.w, r.b, r.go, torch.float32)
    for a, b in ((y32, r.y), (gx32, r.gx), (gw32, r.gw), (gb32, r.gb)):
        assert a.dtype == torch.float32 and torch.equal(a.double(), b)
    # the data exercises what it is meant to: a ReLU mask that is neither empty nor full, nonzero gradients everywhere
    if c.relu:
        pos = float((r.y > 0).double().mean())
        assert 0.2 < pos < 0.8, pos
    assert float(r.gw.abs().amax(dim=(0, 1)).min()) > 0 and bool((r.gb != 0).any())   # every tap


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_faults_change_the_reference(cid):
    """(fp32: equal to float64 on these operands, see above)"""
    c, r = _case(cid), R.reference(cid)
    x, w, b, go = [t.float() for t in (r.x, r.w, r.b, r.go)]
    y = r.y.float()

    def fwd(x_, w_):
        out = R.conv_op(c, x_, w_, b)
        return torch.relu(out) if c.relu else out
    # one tap of w dropped: a corner tap, and the centre
    for ky, kx in ((0, 0), (c.k - 1, c.k - 1), (c.k // 2, c.k // 2)):
        w2 = w.clone()
        w2[:, :, ky, kx] = 0
        assert not torch.equal(fwd(x, w2), y), (ky, kx)
    # the last real input channel dropped (the last 8-channel chunk of a 136-lane buffer, channel 17 of 24, ...)
    x2 = x.clone()
    x2[:, c.cin_w - 1] = 0
    assert not torch.equal(fwd(x2, w), y)
    # the output phase of the transposed conv shifted by one row / column
    if c.transposed:
        assert not torch.equal(torch.roll(y, 1, 2), y) and not torch.equal(torch.roll(y, 1, 3), y)
    # the last output row lost: in y, and its share of the weight gradient
    assert bool((y[:, :, -1] != 0).any())
    go_last = torch.zeros_like(go)
    go_last[:, :, -1] = go[:, :, -1]
    gw_last = R.run_ref(c, x, w, b, go_last, torch.float32)[2]
    assert bool((gw_last != 0).any())
