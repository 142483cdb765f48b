"""GPU: ops.masked_l1_multi (dis_masked_l1_multi_fwd / _bwd, csrc/pixel_ops.hip) against the numpy restatement
tests/masked_l1_ref.py: bit for bit on dyadic inputs (every fp64 sum is exact whatever its order), gradients bit for bit and values
within one float32 ulp on random floats, run-to-run identity, agreement with ops.l1_mean on a hole-free target, and capture."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import masked_l1_ref as R

# (3, 5, 7): the window is larger than what is left of the image; (8, 37, 129): several workgroups, W no multiple of 64;
# (16, 216, 256): 884736 elements over the 1024 workgroups of the accumulate launch - each takes several strides
SHAPES = [(3, 5, 7), (8, 37, 129), (16, 216, 256)]
GS = [1.0, 0.5, 0.25, 3.0]


def _ulp_apart(a, b):
    """distance of two finite float32 in units in the last place"""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    ia, ib = (i if i >= 0 else -(i & 0x7fffffff) for i in (ia, ib))
    return abs(ia - ib)


def _holes(rng, planes, h, w, layout):
    if layout in ('corners', 'last_row_plane0', 'all_hole_plane', 'all_holes'):
        return R.hole_layouts(planes, h, w)[layout]
    m = np.zeros((planes, h, w), dtype=bool)
    if layout == 'random':            # ~30 % holes: rectangles plus single pixels
        for p in range(planes):
            for _ in range(3):
                y, x = rng.randint(0, h), rng.randint(0, w)
                m[p, y:y + rng.randint(1, max(2, h // 3)), x:x + rng.randint(1, max(2, w // 3))] = True
        m |= rng.rand(planes, h, w) < 0.05
    return m


def _run(outs, t, r, gs=None, shape=None):
    """ops.masked_l1_multi on the device -> (values: list of np.float32, grads: list of arrays)"""
    from depthinspace_amd import ops
    shape = shape or outs[0].shape
    od = [torch.from_numpy(o.reshape(shape)).cuda().requires_grad_(True) for o in outs]
    vals = ops.masked_l1_multi(od, torch.from_numpy(t.reshape(shape)).cuda(), r)
    assert len(vals) == len(outs) and all(v.shape == () and v.dtype == torch.float32 for v in vals)
    gs = GS[:len(outs)] if gs is None else gs
    sum(v * g for v, g in zip(vals, gs)).backward()
    torch.cuda.synchronize()
    return [np.float32(v.item()) for v in vals], [o.grad.cpu().numpy() for o in od]


def _bits_equal(got, want):
    for a, b in zip(got[0], want[0]):
        assert np.float32(a).tobytes() == np.float32(b).tobytes(), (a, b)
    for a, b in zip(got[1], want[1]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), float(np.abs(a - b).max())


_CASES = {}


def _dyadic_case(shape, layout):
    key = (shape, layout)
    if key not in _CASES:
        planes, h, w = shape
        rng = np.random.RandomState(planes * 1000 + h + len(layout))
        t = (np.abs(R.dyadic(rng, (planes, 1, h, w))) + np.float32(1 / 64)).astype(np.float32)
        outs = [R.dyadic(rng, (planes, 1, h, w)) for _ in range(4)]
        outs[0][0, 0, h // 2, w // 2] = t[0, 0, h // 2, w // 2]       # sign(0) = 0
        hm = _holes(rng, planes, h, w, layout)
        t = R.punch(t, hm)
        if layout == 'random':
            t[0, 0, 0, 1] = np.nan                                    # a NaN target pixel: a hole
            t[-1, 0, h - 1, w - 2] = -2.0                             # negative: a hole
            outs[1][hm.reshape(t.shape)] = np.inf                     # inf under every hole: a select, not a multiply
            outs[2][0, 0, 0, 1] = np.nan
        _CASES[key] = (outs, t, {})
    return _CASES[key]


# every shape without holes and with random ones (NaN, negative and inf-under-hole pixels among them); the fixed layouts of the CPU
# test on its shape, (3, 5, 7)
DYADIC = [(s, l) for s in SHAPES for l in ('none', 'random')] + \
         [(SHAPES[0], l) for l in ('corners', 'last_row_plane0', 'all_hole_plane', 'all_holes')]


@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('r', [0, 1, 3])
@pytest.mark.parametrize('shape,layout', DYADIC)
def test_dyadic_inputs_bit_for_bit(shape, layout, r, n):
    outs, t, refs = _dyadic_case(shape, layout)
    if (r, n) not in refs:
        refs[(r, n)] = R.masked_l1_multi(outs[:n], t, r, GS[:n])
    want = refs[(r, n)]
    got = _run(outs[:n], t, r)
    _bits_equal(got, want)
    if layout == 'all_holes':
        assert want[2] == 0 and all(v == 0 for v in got[0]) and all(not g.any() for g in got[1])
    elif layout == 'random':
        assert 0 < want[2] < t.size and all(np.isfinite(v) for v in got[0]) and all(np.isfinite(g).all() for g in got[1])


@pytest.mark.parametrize('r', [0, 1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_random_floats(shape, r):
    planes, h, w = shape
    rng = np.random.RandomState(h * w + r)
    t = (rng.rand(planes, 1, h, w) * 60 + 0.5).astype(np.float32)
    t = R.punch(t, _holes(rng, planes, h, w, 'random'))
    outs = [(t + rng.randn(planes, 1, h, w) * (k + 1)).astype(np.float32) for k in range(4)]
    want = R.masked_l1_multi(outs, t, r, GS)
    got = _run(outs, t, r)
    for a, b in zip(got[1], want[1]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got[0], want[0]):
        print(shape, r, a, b, _ulp_apart(a, b))
        assert _ulp_apart(a, b) <= 1, (a, b)
    # the (tl, bs, 1, H, W) view of the same memory: the same planes
    if planes % 2 == 0:
        five = _run(outs, t, r, shape=(2, planes // 2, 1, h, w))
        assert [v.tobytes() for v in five[0]] == [v.tobytes() for v in got[0]]
        assert all(a.shape == (2, planes // 2, 1, h, w) and a.tobytes() == b.tobytes() for a, b in zip(five[1], got[1]))


def test_two_calls_give_the_same_bits():
    planes, h, w = SHAPES[2]
    rng = np.random.RandomState(9)
    t = R.punch((rng.rand(planes, 1, h, w) * 60 + 0.5).astype(np.float32), _holes(rng, planes, h, w, 'random'))
    outs = [(t + rng.randn(planes, 1, h, w)).astype(np.float32) for _ in range(4)]
    a, b = _run(outs, t, 1), _run(outs, t, 1)
    _bits_equal(a, b)


@pytest.mark.parametrize('shape', SHAPES)
def test_hole_free_target_agrees_with_l1_mean(shape):
    from depthinspace_amd import ops
    planes, h, w = shape
    rng = np.random.RandomState(planes + w)
    t = (rng.rand(planes, 1, h, w) * 60 + 0.5).astype(np.float32)
    outs = [(t + rng.randn(planes, 1, h, w) * (k + 1)).astype(np.float32) for k in range(4)]
    got = _run(outs, t, 0)
    td = torch.from_numpy(t).cuda()
    for k in range(4):
        od = torch.from_numpy(outs[k]).cuda().requires_grad_(True)
        v = ops.l1_mean(od, td)
        (v * GS[k]).backward()
        assert _ulp_apart(got[0][k], np.float32(v.item())) <= 1, (got[0][k], v.item())
        assert got[1][k].tobytes() == od.grad.cpu().numpy().tobytes()      # both are +-gscale / (float)count


def test_rejects_bad_arguments():
    from depthinspace_amd import ops, lib
    t = torch.ones(2, 1, 4, 5, device='cuda')
    o = torch.zeros(2, 1, 4, 5, device='cuda')
    with pytest.raises(RuntimeError):
        ops.masked_l1_multi([o] * 5, t)
    with pytest.raises(RuntimeError):
        ops.masked_l1_multi([], t)
    with pytest.raises(RuntimeError):
        ops.masked_l1_multi([o], t, erode=4)
    with pytest.raises(RuntimeError):
        ops.masked_l1_multi([o, torch.zeros(2, 1, 4, 6, device='cuda')], t)
    with pytest.raises(RuntimeError):
        ops.masked_l1_multi([torch.zeros(2, 2, 4, 5, device='cuda')], torch.ones(2, 2, 4, 5, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.masked_l1_multi([torch.zeros(2, 1, 4, 5)], torch.ones(2, 1, 4, 5))     # CPU tensors: no fallback
    f, b = lib.fn('dis_masked_l1_multi_fwd'), lib.fn('dis_masked_l1_multi_bwd')
    acc = torch.empty(lib.fn('dis_masked_l1_multi_acc_doubles')(), dtype=torch.float64, device='cuda')
    out = torch.empty(4, device='cuda')
    import ctypes
    tab, null_tab = ops._ptr_table([o]), (ctypes.c_void_p * 1)(None)
    tp = ctypes.cast(tab, ctypes.c_void_p)
    assert f(None, 1, t.data_ptr(), 0, acc.data_ptr(), out.data_ptr(), 2, 4, 5, None) == -3
    assert f(tp, 1, None, 0, acc.data_ptr(), out.data_ptr(), 2, 4, 5, None) == -3
    assert f(ctypes.cast(null_tab, ctypes.c_void_p), 1, t.data_ptr(), 0, acc.data_ptr(), out.data_ptr(), 2, 4, 5, None) == -3
    for n, r, p, h, w in ((0, 0, 2, 4, 5), (5, 0, 2, 4, 5), (1, -1, 2, 4, 5), (1, 4, 2, 4, 5), (1, 0, 0, 4, 5), (1, 0, 2, 0, 5), (1, 0, 2, 4, -1)):
        assert f(tp, n, t.data_ptr(), r, acc.data_ptr(), out.data_ptr(), p, h, w, None) == -1, (n, r, p, h, w)
        assert b(tp, n, t.data_ptr(), r, acc.data_ptr(), out.data_ptr(), tp, p, h, w, None) == -1, (n, r, p, h, w)
    assert b(tp, 1, t.data_ptr(), 0, acc.data_ptr(), None, tp, 2, 4, 5, None) == -3
    assert b(tp, 1, t.data_ptr(), 0, acc.data_ptr(), out.data_ptr(), None, 2, 4, 5, None) == -3


def test_capture_and_replay_track_the_restatement():
    """the call inside torch.cuda.graph: three replays with changed input contents, then an all-hole target - zeros, not NaN"""
    from depthinspace_amd import ops
    planes, h, w = SHAPES[1]
    rng = np.random.RandomState(21)

    def draw(all_holes=False):
        t = (np.abs(R.dyadic(rng, (planes, 1, h, w))) + np.float32(1 / 64)).astype(np.float32)
        t = R.punch(t, _holes(rng, planes, h, w, 'all_holes' if all_holes else 'random'))
        return [R.dyadic(rng, (planes, 1, h, w)) for _ in range(4)], t

    outs, t = draw()
    od = [torch.from_numpy(o).cuda().requires_grad_(True) for o in outs]
    td = torch.from_numpy(t).cuda()
    gsc = torch.tensor(GS, device='cuda')
    vals_s = torch.zeros(4, device='cuda')
    grads_s = [torch.zeros_like(o) for o in od]

    def step():
        vals = ops.masked_l1_multi(od, td, 1)
        gr = torch.autograd.grad((torch.stack(vals) * gsc).sum(), od)
        vals_s.copy_(torch.stack(vals).detach())
        for d, g in zip(grads_s, gr):
            d.copy_(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in range(4):
        outs, t = draw(all_holes=(k == 3))
        with torch.no_grad():
            for d, o in zip(od, outs):
                d.copy_(torch.from_numpy(o))
            td.copy_(torch.from_numpy(t))
        graph.replay()
        torch.cuda.synchronize()
        want = R.masked_l1_multi(outs, t, 1, GS)
        got = ([np.float32(v) for v in vals_s.cpu().numpy()], [g.cpu().numpy() for g in grads_s])
        _bits_equal(got, want)
        if k == 3:
            assert want[2] == 0 and not vals_s.cpu().numpy().any() and all(not g.any() for g in got[1])
