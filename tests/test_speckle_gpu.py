"""GPU: ops.speckle_filter (csrc/speckle.hip) against the numpy restatement tests/speckle_ref.py - out, label and size equal bit for
bit on every case: labels and counts are integers and the kept pixels are copies.  The shapes cross the kernels' 64 x 16 tile in both
directions and leave tiles partly empty; the serpentine and the spiral are the longest parent chains the union-find can meet."""
import functools

import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import speckle_ref

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _gpu(d, max_size, max_diff, **kw):
    from depthinspace_amd import ops
    out, dbg = ops.speckle_filter(torch.from_numpy(np.ascontiguousarray(d, dtype=F)).cuda(), max_size, max_diff, want_debug=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dbg['label'].cpu().numpy(), dbg['size'].cpu().numpy()


def _check(d, max_size, max_diff, ref=None):
    """the kernels on d (n, h, w) against the restatement (or its result `ref` for this d and max_diff, any max_size)"""
    d = np.ascontiguousarray(d, dtype=F)
    if ref is None:
        ref = speckle_ref.speckle_filter(d, max_size, max_diff)
    _, label, size = ref
    want = np.where(size > max_size, d, F(0))
    out, got_label, got_size = _gpu(d, max_size, max_diff)
    assert out.shape == d.shape and out.dtype == F
    assert np.array_equal(got_label, label), np.argwhere(got_label != label)[:5]
    assert np.array_equal(got_size, size), np.argwhere(got_size != size)[:5]
    assert np.array_equal(_bits(out), _bits(want)), np.argwhere(_bits(out) != _bits(want))[:5]
    return out, label, size


@functools.lru_cache(maxsize=None)
def _random_case(shape, max_diff):
    rng = np.random.RandomState(shape[1] + shape[2])
    d = rng.choice(np.array([0, 5, 6, 7, 20], F), size=shape).astype(F)
    return d, speckle_ref.speckle_filter(d, 0, max_diff)


@pytest.mark.parametrize('max_diff', [0.0, 1.0, 2.5])
@pytest.mark.parametrize('shape', [(3, 70, 133), (3, 33, 257)], ids=['70x133', '33x257'])
def test_random_integer_disparities(shape, max_diff):
    d, ref = _random_case(shape, max_diff)
    sizes = ref[2]
    assert len(np.unique(sizes)) > (3 if max_diff == 0 else 8)      # components of many sizes
    for max_size in (0, 1, 7, 100, 10 ** 6):
        out, _, _ = _check(d, max_size, max_diff, ref)
        if max_size == 0:
            assert np.array_equal(out, d)
        if max_size == 10 ** 6:
            assert not out.any()
    # (n, 1, H, W) gives the same planes in that shape
    from depthinspace_amd import ops
    o4 = ops.speckle_filter(torch.from_numpy(d[:, None]).cuda(), 7, max_diff)
    assert tuple(o4.shape) == (shape[0], 1) + shape[1:]
    assert np.array_equal(o4.cpu().numpy()[:, 0], np.where(sizes > 7, d, F(0)))


def serpentine(h=64, w=96):
    """one path through every second row, joined at alternating ends by one pixel of the row between; the disparity grows by 0.5 per
    pixel along the path (every value exact in fp32), so max_diff = 0.5 links the path and nothing else"""
    d = np.zeros((h, w), F)
    k = 0
    for y in range(0, h, 2):
        xs = range(w) if (y // 2) % 2 == 0 else range(w - 1, -1, -1)
        for x in xs:
            d[y, x] = 1 + 0.5 * k
            k += 1
        if y + 2 < h:
            d[y + 1, xs[-1]] = 1 + 0.5 * k
            k += 1
    return d, k


@pytest.mark.parametrize('transpose', [False, True], ids=['rows', 'columns'])
def test_serpentine_is_one_component(transpose):
    d, k = serpentine()
    assert k == 32 * 96 + 31
    d = d.T.copy() if transpose else d
    out, label, size = _check(d[None], k - 1, 0.5)
    assert (label[0][d > 0] == 0).all() and (size[0][d > 0] == k).all() and np.array_equal(out[0], d)
    assert not _check(d[None], k, 0.5)[0].any()


def spiral(n=65):
    """a path from the corner inwards with one invalid pixel between its arms; 0.25 more disparity per pixel along it"""
    d = np.zeros((n, n), F)
    y = x = 0
    dy, dx = 0, 1
    k = 0
    d[0, 0] = 2
    while True:
        for _ in range(2):
            ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and d[ny, nx] == 0 and not (0 <= my < n and 0 <= mx < n and d[my, mx] != 0):
                break
            dy, dx = dx, -dy                           # turn right
        else:
            return d, k + 1
        y, x, k = ny, nx, k + 1
        d[y, x] = 2 + 0.25 * k


def test_spiral():
    d, k = spiral()
    assert k > 2000
    out, label, size = _check(d[None], k - 1, 0.25)
    assert (label[0][d > 0] == 0).all() and (size[0][d > 0] == k).all() and np.array_equal(out[0], d)
    assert not _check(d[None], k, 0.25)[0].any()


def test_checkerboard_is_all_singletons():
    y, x = np.mgrid[0:37, 0:70]
    d = np.where((x + y) % 2 == 0, F(3), F(9))[None]
    out, label, size = _check(d, 0, 1.0)
    assert (size == 1).all() and np.array_equal(label[0], y * 70 + x) and np.array_equal(out, d)
    assert not _check(d, 1, 1.0)[0].any()


def test_uniform_image_is_one_component():
    d = np.full((2, 50, 130), 11.5, F)
    out, label, size = _check(d, 50 * 130 - 1, 0.0)
    assert (label == 0).all() and (size == 50 * 130).all() and np.array_equal(out, d)
    assert not _check(d, 50 * 130, 0.0)[0].any()


@pytest.mark.parametrize('shape', [(1, 300), (300, 1), (1, 1), (2, 2)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_thin_images(shape):
    rng = np.random.RandomState(shape[0] + 7 * shape[1])
    d = rng.choice(np.array([0, 5, 6, 20], F), size=(2,) + shape).astype(F)
    d[0].flat[0] = 5                                   # (at least one valid pixel)
    for max_size in (0, 1, 3):
        _check(d, max_size, 1.0)
    _check(np.full((1,) + shape, 4, F), shape[0] * shape[1] - 1, 0.0)


def test_comb_joined_in_the_last_row_and_column():
    h, w = 40, 131
    d = np.zeros((2, h, w), F)
    d[0, :, 0::2] = 5                                   # teeth down the columns: no two of them are neighbours ...
    d[0, -1, :] = 5                                     # ... they meet in the last row only
    d[1, 0::2, :] = 5                                   # teeth along the rows ...
    d[1, :, -1] = 5                                     # ... that meet in the last column only
    out, label, size = _check(d, 100, 1.0)
    ok = d > 0
    assert (label[ok] == 0).all() and (size[0][ok[0]] == ok[0].sum()).all() and (size[1][ok[1]] == ok[1].sum()).all()
    # the teeth alone, joined by nothing: each its own component, first pixel at the top
    t = np.zeros((1, h, w), F)
    t[0, :, 0::2] = 5
    out, label, size = _check(t, h - 1, 1.0)
    assert np.array_equal(label[0][:, 0::2], np.broadcast_to(np.arange(0, w, 2), (h, 66))) and np.array_equal(out, t)
    assert not _check(t, h, 1.0)[0].any()


def test_values_that_are_not_disparities():
    from tests.test_speckle_ref_cpu import bad_values_image
    small = bad_values_image()
    out, label, size = _check(small[None], 3, 1.0)
    assert (out[0][~speckle_ref.valid_mask(small)].view(np.uint32) == 0).all()      # +0.0, whatever stood there
    big = np.tile(small, (20, 11))                       # 40 x 143: the same values across tile borders
    for max_size in (0, 4, 50):
        _check(np.stack([big, big[::-1]]), max_size, 1.0)


def test_images_of_a_batch_are_independent():
    d1, _ = _random_case((3, 70, 133), 1.0)
    d = np.stack([d1[0], d1[0]])
    out, label, size = _check(d, 7, 1.0)
    assert np.array_equal(out[0], out[1]) and np.array_equal(label[0], label[1]) and np.array_equal(size[0], size[1])
    assert label.min() == -1 and label.max() < 70 * 133
    # a component that ends in the last row of one image does not go on in the first row of the next
    e = np.zeros((2, 17, 64), F)
    e[0, -1] = 5
    e[1, 0] = 5
    out, label, size = _check(e, 64, 1.0)
    assert (size[0, -1] == 64).all() and (size[1, 0] == 64).all() and not out.any()


def test_workspace_reuse_and_no_initialisation():
    from depthinspace_amd import ops, lib
    d, ref = _random_case((3, 70, 133), 1.0)
    need = lib.fn('dis_speckle_workspace')(3, 70, 133)
    assert need >= 3 * 70 * 133 * 8
    x = torch.from_numpy(d).cuda()
    fresh, dbg0 = ops.speckle_filter(x, 7, 1.0, want_debug=True)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    ws.fill_(0xff)
    a, dbg_a = ops.speckle_filter(x, 7, 1.0, want_debug=True, workspace=ws)
    b, dbg_b = ops.speckle_filter(x, 7, 1.0, want_debug=True, workspace=ws)      # what the first call left in it
    c, dbg_c = ops.speckle_filter(x, 100, 2.5, want_debug=True, workspace=ws)    # another configuration on the same workspace
    e, dbg_e = ops.speckle_filter(x, 7, 1.0, want_debug=True, workspace=ws)
    torch.cuda.synchronize()
    for o, g in ((a, dbg_a), (b, dbg_b), (e, dbg_e)):
        assert torch.equal(o.view(torch.int32), fresh.view(torch.int32))
        assert torch.equal(g['label'], dbg0['label']) and torch.equal(g['size'], dbg0['size'])
    assert np.array_equal(fresh.cpu().numpy(), np.where(ref[2] > 7, d, F(0)))
    _, ref25 = _random_case((3, 70, 133), 2.5)
    assert np.array_equal(c.cpu().numpy(), np.where(ref25[2] > 100, d, F(0))) and np.array_equal(dbg_c['size'].cpu().numpy(), ref25[2])
    with pytest.raises(lib.DisHipError):
        ops.speckle_filter(x, 7, 1.0, workspace=ws[:need - 16])
    with pytest.raises(lib.DisHipError):
        ops.speckle_filter(x, 7, 1.0, workspace=torch.empty(need + 16, dtype=torch.uint8, device='cuda')[1:])
    with pytest.raises(RuntimeError):
        ops.speckle_filter(x, 7, 1.0, workspace=torch.empty(need, dtype=torch.float32, device='cuda'))


def test_graph_capture_on_a_side_stream():
    from depthinspace_amd import ops, lib
    d, ref = _random_case((3, 70, 133), 1.0)
    want = np.where(ref[2] > 7, d, F(0))
    x = torch.full((3, 70, 133), 5.0, device='cuda')
    ws = torch.empty(lib.fn('dis_speckle_workspace')(3, 70, 133), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.speckle_filter(x, 7, 1.0, workspace=ws)
    x.copy_(torch.from_numpy(d))                        # the capture executed nothing: the replay sees the changed input
    graph.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    ws.fill_(0xff)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(first), _bits(want)) and np.array_equal(_bits(out.cpu().numpy()), _bits(want))


def test_bad_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    x = torch.full((1, 16, 70), 5.0, device='cuda')
    for kw in (dict(max_size=-1), dict(max_diff=-1.0), dict(max_diff=float('nan')), dict(max_diff=float('inf')),
               dict(max_diff=1e39)):
        with pytest.raises(lib.DisHipError):
            ops.speckle_filter(x, **kw)
    for bad in (torch.zeros(16, 70, device='cuda'), torch.zeros(1, 2, 16, 70, device='cuda'), torch.zeros(1, 1, 1, 16, 70, device='cuda')):
        with pytest.raises(RuntimeError):
            ops.speckle_filter(bad)
    with pytest.raises(RuntimeError):
        ops.speckle_filter(torch.zeros(1, 16, 70))                                  # a CPU tensor
    with pytest.raises(RuntimeError):
        ops.speckle_filter(torch.zeros(1, 16, 70, device='cuda', dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.speckle_filter(torch.zeros(1, 16, 140, device='cuda')[:, :, ::2])       # not contiguous
    # and by the entry point itself (the python wrapper checks first): a sentinel output stays untouched
    ws = torch.empty(lib.fn('dis_speckle_workspace')(1, 16, 70), dtype=torch.uint8, device='cuda')
    out = torch.full((1, 16, 70), -7.0, device='cuda')
    for max_size, max_diff in ((-1, 1.0), (5, -1.0), (5, float('nan')), (5, float('inf'))):
        with pytest.raises(lib.DisHipError):
            lib.call('dis_speckle_filter', x, out, None, None, 1, 16, 70, max_size, max_diff, ws)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_speckle_filter', x, out, None, None, 1, 16, 70, 5, 1.0, ws[1:])     # misaligned workspace
    with pytest.raises(lib.DisHipError):
        lib.call('dis_speckle_filter', x, out, None, None, 1, 0, 70, 5, 1.0, ws)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_speckle_filter', x, None, None, None, 1, 16, 70, 5, 1.0, ws)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    W = lib.fn('dis_speckle_workspace')
    assert W(1, 9000, 70) == -1 and W(0, 16, 70) == -1 and W(1, 16, 0) == -1 and W(64, 8192, 8192) == -1 and W(31, 8192, 8192) > 0
