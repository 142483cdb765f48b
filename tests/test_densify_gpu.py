"""GPU: ops.disp_densify (csrc/densify.hip) against the numpy restatement tests/densify_ref.py - out and state equal bit for bit on
every case: both stages only select and compare.  The shapes leave the kernels' 64 x 16 tiles ragged in both axes and span several of
them; a gap of 32 makes the halo two tile rows deep, and at 17 x 65 wider than the image."""
import itertools

import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import densify_ref

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = densify_ref.FLT_MAX


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _gpu(d, max_gap, min_dirs, max_spread, median_r, **kw):
    from depthinspace_amd import ops
    out, state = ops.disp_densify(torch.from_numpy(np.ascontiguousarray(d, dtype=F)).cuda(), max_gap, min_dirs, max_spread, median_r,
                                  want_state=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), state.cpu().numpy()


def _same(got, want, what):
    out, state = got
    ref_out, ref_state = want
    assert out.shape == ref_out.shape and out.dtype == F and state.dtype == np.uint8
    assert np.array_equal(state, ref_state), (what, np.argwhere(state != ref_state)[:5])
    assert np.array_equal(_bits(out), _bits(ref_out)), (what, np.argwhere(_bits(out) != _bits(ref_out))[:5])


def _check(d, max_gap, min_dirs, max_spread, median_r):
    d = np.ascontiguousarray(d, dtype=F)
    want = densify_ref.disp_densify(d, max_gap, min_dirs, max_spread, median_r)
    _same(_gpu(d, max_gap, min_dirs, max_spread, median_r), want, (max_gap, min_dirs, max_spread, median_r))
    return want


def random_maps(shape, seed=0):
    """six maps per image of `shape`, stacked along n (the images of a batch are independent): integer disparities from {5, 6, 7, 20}
    and uniform floats, each at the densities 0.3, 0.6 and 0.9"""
    rng = np.random.RandomState(seed + shape[1] + 3 * shape[2])
    maps = []
    for density in (0.3, 0.6, 0.9):
        keep = rng.rand(*shape) < density
        maps.append(np.where(keep, rng.choice(np.array([5, 6, 7, 20], F), size=shape), 0))
        maps.append(np.where(keep, rng.uniform(1, 60, size=shape), 0))
    return np.concatenate(maps).astype(F)


SHAPES = [(1, 1, 1), (1, 1, 200), (1, 50, 1), (3, 17, 65), (2, 33, 130), (2, 40, 56)]


@pytest.mark.parametrize('max_gap', [0, 1, 8, 16, 32])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_random_maps(shape, max_gap):
    """every min_dirs of {1, 6, 8}, max_spread of {0, 2, FLT_MAX} and median_r of {0, 1, 2}: the fill alone (r = 0), the median alone
    (gap 0) and both together.  The fill of the restatement is computed once per (min_dirs, max_spread) and the median applied to it."""
    d = random_maps(shape)
    clean = np.where(densify_ref.valid_mask(d), d, F(0)).astype(F)
    gates = [(6, 2.0)] if max_gap == 0 else list(itertools.product((1, 6, 8), (0.0, 2.0, FLT_MAX)))
    some_fill = some_gate = False
    for min_dirs, max_spread in gates:
        stage1, state = densify_ref.fill(clean, max_gap, min_dirs, max_spread)
        some_fill = some_fill or bool((state == 2).any())
        some_gate = some_gate or (max_spread == 0.0 and bool(((state == 0) & (densify_ref.fill(clean, max_gap, min_dirs, FLT_MAX)[1] == 2)).any()))
        for r in (0, 1, 2):
            _same(_gpu(d, max_gap, min_dirs, max_spread, r), (densify_ref.median(stage1, r), state), (min_dirs, max_spread, r))
    if max_gap > 0 and shape[1] * shape[2] > 1:
        assert some_fill and some_gate                  # the cases do fill, and the gate does refuse


def test_four_dimensional_input_and_no_state():
    from depthinspace_amd import ops
    d = random_maps((2, 33, 130))
    want, _ = densify_ref.disp_densify(d, 16, 6, 2.0, 1)
    out = ops.disp_densify(torch.from_numpy(d[:, None]).cuda())                        # the defaults are 16, 6, 2.0, 1
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (d.shape[0], 1, 33, 130)
    assert np.array_equal(_bits(out.cpu().numpy()[:, 0]), _bits(want))


def test_rays_of_exactly_max_gap_across_tiles():
    """one valid pixel: the 8 rays of max_gap pixels around it, through up to three tiles, and not one pixel more"""
    d = np.zeros((1, 80, 200), F)
    d[0, 40, 100] = 7
    for gap in (1, 16, 31, 32):
        out, state = _check(d, gap, 1, 0.0, 0)
        assert (out != 0).sum() == 8 * gap + 1
        for dy, dx in densify_ref.DIRECTIONS:
            assert out[0, 40 + gap * dy, 100 + gap * dx] == 7 and state[0, 40 + gap * dy, 100 + gap * dx] == 2
            assert out[0, 40 + (gap + 1) * dy, 100 + (gap + 1) * dx] == 0
    # the same from the image's corners, where the rays start in the halo's far cells
    c = np.zeros((1, 33, 65), F)
    c[0, 0, 0] = c[0, 32, 64] = 3
    c[0, 0, 64] = c[0, 32, 0] = 4
    out, state = _check(c, 8, 1, FLT_MAX, 0)
    assert out[0, 8, 8] == 3 and out[0, 24, 56] == 3 and out[0, 8, 56] == 4 and out[0, 24, 8] == 4
    out, state = _check(c, 32, 1, FLT_MAX, 0)
    assert out[0, 32, 32] == 3 and out[0, 0, 32] == 3      # 3 from the diagonal and along the row, 4 along the row: 3 3 4


def test_hole_across_a_tile_corner():
    """a 4 x 4 hole over the corner where four tiles meet, in a map of distinct values: every walk of its pixels crosses a tile border,
    all four diagonals included, and the medians tell the directions apart"""
    y, x = np.mgrid[0:48, 0:160]
    d = (1 + (y * 160 + x) * F(2.0 ** -8)).astype(F)[None]
    d[0, 14:18, 62:66] = 0
    for gap, dirs in [(1, 1), (3, 5), (4, 8), (32, 8)]:
        for r in (0, 1, 2):
            out, state = _check(d, gap, dirs, FLT_MAX, r)
        assert (state[0, 14:18, 62:66] == 2).sum() == {(1, 1): 12, (3, 5): 16, (4, 8): 16, (32, 8): 16}[(gap, dirs)]
    assert (_check(d, 4, 8, 2.0, 0)[1][0, 14:18, 62:66] == 0).all()                    # N and S differ by 5 rows of 160 / 256


def test_values_that_are_not_disparities():
    from tests.test_speckle_ref_cpu import bad_values_image
    small = bad_values_image()
    out, state = _check(small[None], 0, 1, 0.0, 0)
    assert (_bits(out)[state == 0] == 0).all() and (state == 0).sum() == 10            # +0.0, whatever stood there
    big = np.tile(small, (20, 11))                       # 40 x 143: the same values across tile borders
    both = np.stack([big, big[::-1]])
    for gap, dirs, spread, r in [(0, 1, 0.0, 0), (0, 1, 0.0, 2), (1, 2, 0.0, 0), (1, 8, 0.0, 1), (16, 6, 2.0, 1), (32, 8, FLT_MAX, 2)]:
        out, state = _check(both, gap, dirs, spread, r)
        assert np.isin(_bits(out), _bits(np.array([0, 7], F))).all()
    lone = np.array([[[np.nan, -np.inf, -0.0, -2, np.inf]]], F)
    out, state = _check(lone, 32, 1, FLT_MAX, 2)
    assert (_bits(out) == 0).all() and not state.any()


def test_images_of_a_batch_are_independent():
    e = np.zeros((2, 17, 64), F)
    e[0, 0] = 5                                         # the last row of image 0 is a hole with the first row of image 1 beside it in memory
    e[1, 0] = 9
    out, state = _check(e, 16, 1, 0.0, 0)
    assert (out[0] == 5).all() and (out[1] == 9).all()
    e[1] = 9
    e[0] = 0
    for r in (0, 2):
        out, state = _check(e, 32, 1, FLT_MAX, r)
        assert not out[0].any() and (out[1] == 9).all()
        out, state = _check(e[::-1].copy(), 32, 1, FLT_MAX, r)
        assert not out[1].any() and (out[0] == 9).all()


def test_workspace_reuse_and_no_initialisation():
    from depthinspace_amd import ops, lib
    big, small = random_maps((2, 40, 56)), random_maps((3, 17, 65))
    need = lib.fn('dis_disp_densify_workspace')(*big.shape)
    assert need >= big.size * 4 and need % 16 == 0 and lib.fn('dis_disp_densify_workspace')(*small.shape) <= need
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    ws.fill_(0xff)                                       # every float of it a NaN
    want_big, want_small = densify_ref.disp_densify(big, 16, 6, 2.0, 1), densify_ref.disp_densify(small, 32, 1, FLT_MAX, 2)
    _same(_gpu(big, 16, 6, 2.0, 1, workspace=ws), want_big, 'big')
    _same(_gpu(small, 32, 1, FLT_MAX, 2, workspace=ws), want_small, 'small after big')
    ws.fill_(0xff)
    _same(_gpu(small, 32, 1, FLT_MAX, 2, workspace=ws), want_small, 'small on NaNs')
    _same(_gpu(big, 16, 6, 2.0, 1, workspace=ws), want_big, 'big after small')
    x = torch.from_numpy(big).cuda()
    with pytest.raises(lib.DisHipError):
        ops.disp_densify(x, workspace=ws[:need - 16])
    with pytest.raises(lib.DisHipError):
        ops.disp_densify(x, workspace=torch.empty(need + 16, dtype=torch.uint8, device='cuda')[1:])
    with pytest.raises(RuntimeError):
        ops.disp_densify(x, workspace=torch.empty(need, dtype=torch.float32, device='cuda'))


def test_graph_capture_on_a_side_stream():
    from depthinspace_amd import ops, lib
    d = random_maps((2, 33, 130))
    want = densify_ref.disp_densify(d, 16, 6, 2.0, 1)
    x = torch.full(d.shape, 5.0, device='cuda')
    ws = torch.empty(lib.fn('dis_disp_densify_workspace')(*d.shape), dtype=torch.uint8, device='cuda')
    eager = _gpu(d, 16, 6, 2.0, 1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out, state = ops.disp_densify(x, 16, 6, 2.0, 1, want_state=True, workspace=ws)
    x.copy_(torch.from_numpy(d))                        # the capture executed nothing: the replay sees the changed input
    graph.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy(), state.cpu().numpy()
    ws.fill_(0xff)
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    second = out.cpu().numpy(), state.cpu().numpy()
    _same(first, want, 'first replay')
    _same(second, want, 'second replay')
    _same(eager, want, 'eager')


def test_bad_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    x = torch.full((1, 16, 70), 5.0, device='cuda')
    for kw in (dict(max_gap=33), dict(max_gap=-1), dict(min_dirs=0), dict(min_dirs=9), dict(median=3), dict(median=-1),
               dict(max_spread=-1.0), dict(max_spread=float('nan')), dict(max_spread=float('inf')), dict(max_spread=1e39)):
        with pytest.raises(lib.DisHipError):
            ops.disp_densify(x, **kw)
    for bad in (torch.zeros(16, 70, device='cuda'), torch.zeros(1, 2, 16, 70, device='cuda'), torch.zeros(1, 1, 1, 16, 70, device='cuda')):
        with pytest.raises(RuntimeError):
            ops.disp_densify(bad)
    with pytest.raises(RuntimeError):
        ops.disp_densify(torch.zeros(1, 16, 70))                                    # a CPU tensor
    with pytest.raises(RuntimeError):
        ops.disp_densify(torch.zeros(1, 16, 70, device='cuda', dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.disp_densify(torch.zeros(1, 16, 140, device='cuda')[:, :, ::2])         # not contiguous
    # and by the entry point itself (the python wrapper checks first): sentinel outputs stay untouched
    ws = torch.empty(lib.fn('dis_disp_densify_workspace')(1, 16, 70), dtype=torch.uint8, device='cuda')
    out = torch.full((1, 16, 70), -7.0, device='cuda')
    state = torch.full((1, 16, 70), 9, dtype=torch.uint8, device='cuda')
    for gap, dirs, spread, r in ((33, 6, 2.0, 1), (-1, 6, 2.0, 1), (16, 0, 2.0, 1), (16, 9, 2.0, 1), (16, 6, 2.0, 3), (16, 6, 2.0, -1),
                                 (16, 6, -1.0, 1), (16, 6, float('nan'), 1), (16, 6, float('inf'), 1)):
        with pytest.raises(lib.DisHipError):
            lib.call('dis_disp_densify', x, out, state, 1, 16, 70, gap, dirs, spread, r, ws)
    xb = x.clone()
    with pytest.raises(lib.DisHipError):
        lib.call('dis_disp_densify', x, x, state, 1, 16, 70, 16, 6, 2.0, 1, ws)        # out aliases disp
    with pytest.raises(lib.DisHipError):
        lib.call('dis_disp_densify', x, out, x, 1, 16, 70, 16, 6, 2.0, 1, ws)          # state aliases disp
    with pytest.raises(lib.DisHipError):
        lib.call('dis_disp_densify', x, out, state, 1, 16, 70, 16, 6, 2.0, 1, ws[1:])  # misaligned workspace
    with pytest.raises(lib.DisHipError):
        lib.call('dis_disp_densify', x, out, state, 1, 0, 70, 16, 6, 2.0, 1, ws)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_disp_densify', x, None, state, 1, 16, 70, 16, 6, 2.0, 1, ws)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_disp_densify', x, out, state, 1, 16, 70, 16, 6, 2.0, 1, None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((state == 9).all()) and torch.equal(x, xb)
    W = lib.fn('dis_disp_densify_workspace')
    assert W(1, 9000, 70) == -1 and W(0, 16, 70) == -1 and W(1, 16, 0) == -1 and W(64, 8192, 8192) == -1 and W(31, 8192, 8192) > 0
