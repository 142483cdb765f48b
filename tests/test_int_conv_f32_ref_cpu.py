"""The case table, operands and reference of tests/int_conv_f32_ref.py, checked on the CPU: what tests/test_convg_exact_gpu.py relies on.

Per case: the three L1 bounds hold (< 2^24); the fp32 CPU run equals the float64 one (so the fp32 host reference of the ref32 cases
is the float64 reference); the EMULATED two-term fp16 split - one power-of-two scale per image / per weight tensor, h1 = fp16(v s),
h2 = fp16(v s - h1), three products a1 b1 + a1 b2 + a2 b1 - equals float64 for the forward, the input gradient and the weight
gradient, and the dropped a2 b2 part is identically zero; the wide values reach a border pixel of the last row and the last channel
chunk; the ReLU mask is neither empty nor full; every tap of gw carries data.  And the faults the method is for CHANGE the emulated
result - among them the two a tolerance of 2e-5 cannot see: the second plane of x zeroed in the last column, the second plane of w
zeroed for the last tap.  The emulation accumulates in float64 (fp32 for the ref32 cases, whose sums the bounds make exact: float64
would take minutes); the per-fault loop leaves out the cases marked faults=False (the large ones) for host time."""
import pytest
import torch
import torch.nn.functional as F

from tests import int_conv_f32_ref as R


def _wide(t):
    return t.abs() == R.WIDE


def _last_chunk(c_real, ck, parity):
    """channels of the last chunk of ck that holds a channel of the given parity (0 even, 1 odd)"""
    last = (c_real - 1 - parity) // 2 * 2 + parity
    return slice(last // ck * ck, c_real)


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_case_table(cid):
    c = R.case(cid)
    assert c.n >= 2 and c.cin_mem % 4 == 0 and c.cin_w <= c.cin_mem and c.cout % 4 == 0
    x, w, b, go = R.make_inputs(c)
    ck = 32 if c.cin_mem >= 32 else 16
    # ---- placement: no product has two wide factors ----
    wx, wg, ww = _wide(x), _wide(go), _wide(w)
    assert not bool(wx[1:].any()) and not bool(wx[:, 1::2].any())
    assert not bool(wg[0].any()) and not bool(wg[2:].any()) and not bool(wg[:, 1::2].any())
    wwc = ww.transpose(0, 1) if c.transposed else ww          # (cout, cin, k, k)
    assert not bool(wwc[0::2].any()) and not bool(wwc[:, 0::2].any())
    for t in (x, go, w):
        assert float(t[~_wide(t)].abs().max()) <= 2 and bool((t == t.round()).all())
    # ---- the wide values reach a border pixel of the last row, and the last chunk ----
    assert bool(wx[0, _last_chunk(c.cin_w, ck, 0), -1, :].any()) and bool(wx[0, :, :, -1].any()) and bool(wx[0, :, 0, :].any())
    cko = 32 if c.cout >= 32 else 16
    assert bool(wg[1, _last_chunk(c.cout, cko, 0), -1, :].any()) and bool(wg[1, :, :, -1].any())
    assert bool(wwc[:, _last_chunk(c.cin_w, ck, 1), -1, -1].any()) and bool(wwc[_last_chunk(c.cout, cko, 1), :, 0, 0].any())
    # ---- bounds, fp32 == fp64 ----
    yb, gxb, gwb = R.bounds(c, x, w, b, go, torch.float32 if c.ref32 else torch.float64)
    print(f'{cid}: L1 bounds y {yb:.0f} gx {gxb:.0f} gw/gb {gwb:.0f}')
    assert max(yb, gxb, gwb) < R.BOUND, (yb, gxb, gwb)
    y, gx, gw, gb = R.run_ref(c, x, w, b, go)
    for a32, a64 in zip(R.run_ref(c, x, w, b, go, torch.float32), (y, gx, gw, gb)):
        assert torch.equal(a32.double(), a64)
    if c.relu:
        frac = float((y > 0).double().mean())
        assert 0.05 < frac < 0.95, frac
    assert float(gw.abs().amax(dim=(0, 1)).min()) > 0           # every tap carries data
    pre = R.conv_op(c, x, w, b)
    gpre = go * (pre > 0) if c.relu else go
    assert bool(_wide(gpre)[1].any())                           # (wide gradient values survive the ReLU mask)
    # ---- the emulated two-term split: three products equal float64, the fourth is zero ----
    dt = torch.float32 if c.ref32 else torch.float64
    xs, ws, gs = R.split2(x.to(dt), True), R.split2(w.to(dt), False), R.split2(gpre.to(dt), True)
    for t, (h1, h2) in ((x, xs), (w, ws), (gpre, gs)):
        assert torch.equal((h1 + h2).double(), t) and bool((h2 != 0).any())      # the split is exact, the second plane is in use
    e_y, z_y = R.emulate(R.op_fwd, c, xs, ws)
    assert torch.equal(e_y.double() + b.view(1, -1, 1, 1), pre) and not bool(z_y.any())
    e_gw, z_gw = R.emulate(R.op_wgrad, c, xs, gs)
    assert torch.equal(e_gw.double(), gw) and not bool(z_gw.any())
    if c.need_dgrad:
        e_gx, z_gx = R.emulate(R.op_dgrad, c, gs, ws)
        assert torch.equal(e_gx.double(), gx) and not bool(z_gx.any())
    if not c.faults:
        return
    # ---- the faults the method is for change the (emulated) result ----
    k = c.k

    def fwd(xs_, ws_):
        return R.emulate(R.op_fwd, c, xs_, ws_)[0]

    def zero(t, idx):
        t = t.clone()
        t[idx] = 0
        return t
    tap = (Ellipsis, k - 1, k // 2)
    assert not torch.equal(fwd(xs, (zero(ws[0], tap), zero(ws[1], tap))), e_y), 'a dropped tap'
    last = (slice(None), c.cin_w - 1)
    assert not torch.equal(fwd((zero(xs[0], last), zero(xs[1], last)), ws), e_y), 'the last real input channel dropped'
    assert bool((F.relu(pre) if c.relu else pre)[:, :, -1, :].any()), 'a lost last output row'
    assert not torch.equal(fwd((xs[0], zero(xs[1], (Ellipsis, -1))), ws), e_y), 'second plane of x zeroed in the last column'
    assert not torch.equal(fwd(xs, (ws[0], zero(ws[1], (Ellipsis, k - 1, k - 1)))), e_y), 'second plane of w zeroed for the last tap'
    e_gw2 = R.emulate(R.op_wgrad, c, (xs[0], zero(xs[1], (Ellipsis, -1))), gs)[0]
    assert not torch.equal(e_gw2, e_gw), 'weight gradient: second plane of x zeroed in the last column'
    if c.need_dgrad:
        e_gx2 = R.emulate(R.op_dgrad, c, gs, (ws[0], zero(ws[1], (Ellipsis, k - 1, k - 1))))[0]
        assert not torch.equal(e_gx2, e_gx), 'input gradient: second plane of w zeroed for the last tap'
    # a parity phase shifted by one pixel: the forward of a transposed conv, the input gradient of a stride-2 layer
    phased = pre if c.transposed else (gx if c.stride == 2 and c.need_dgrad else None)
    if phased is not None:
        ph = phased[:, :, 1::2, 1::2]
        assert not torch.equal(torch.roll(ph, 1, dims=3), ph), 'a shifted phase'


def test_reference_is_shared_and_fp32_where_stated():
    small = R.reference('g2_tiny')
    assert small is R.reference('g2_tiny') and small.y.dtype == torch.float64
    assert all(R.case(i).ref32 == (i in ('big_sk', 'big_plain', 'sl_16_16', 'sl_48_40', 'sl_16_16_k7')) for i in R.CASE_IDS)
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)
