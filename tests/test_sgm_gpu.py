"""GPU: dis_sgm_disparity (csrc/sgm.hip) against the numpy restatement tests/sgm_ref.py, stage by stage and bit for bit - the census
words, the aggregated volume, the winning candidate, the valid mask and the disparity - plus repeatability, graph capture and the
refusal of unsupported arguments.  Everything up to the winning candidate is integer arithmetic, the sub-pixel term is three exact
fp32 operations and one correctly rounded division: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

from tests import sgm_ref

pytestmark = pytest.mark.gpu

# (n, H, W, ndisp): odd extents with W barely above D; W < D; two and four candidates per lane; Input A's size with 4 frames
SHAPES = [(1, 37, 83, 64), (2, 24, 40, 64), (1, 64, 200, 128), (1, 16, 300, 256), (4, 96, 160, 64)]
INPUTS = ['synth', 'noise', 'quant4', 'const']
PARAMS = [dict(p1=7, p2=60, uniq=5, lr=1), dict(p1=1, p2=127, uniq=0, lr=0)]

_INPUT, _REF = {}, {}


def _input(shape, kind):
    """(im (n, H, W), pattern (H, W)) float32 numpy"""
    key = (shape, kind)
    if key not in _INPUT:
        from depthinspace_amd import synth
        n, H, W, _ = shape
        st = synth.make_settings(H, W, pattern='real')
        pat = np.ascontiguousarray(st.pattern[..., 0], dtype=np.float32)
        if kind in ('synth', 'quant4'):     # Input A of tests/test_sgm_ref_cpu.py at this size: n frames of one track
            scene = 'bumps' if kind == 'synth' else 'plane'
            im = synth.make_batch(st, 1, tl=n, seed=7, scene=scene, with_flow=False, with_primary=False)['im0'][0, :, 0]
            if kind == 'quant4':            # 4 grey levels: the census comparisons are full of exact ties
                im = np.floor(im * 3.999) / 3
                pat = np.floor(pat / max(float(pat.max()), 1e-6) * 3.999) / 3
        elif kind == 'noise':               # no structure: the aggregated costs are full of near-ties
            im = np.random.RandomState(11).rand(n, H, W)
        else:
            im = np.full((n, H, W), 0.5)
        _INPUT[key] = (np.ascontiguousarray(im, dtype=np.float32), np.ascontiguousarray(pat, dtype=np.float32))
    return _INPUT[key]


def _ref(shape, kind, pi):
    key = (shape, kind, pi)
    if key not in _REF:
        im, pat = _input(shape, kind)
        _REF[key] = sgm_ref.sgm_disparity(im, pat, ndisp=shape[3], **PARAMS[pi])
    return _REF[key]


def _run(shape, kind, pi, **kw):
    from depthinspace_amd import ops
    im, pat = _input(shape, kind)
    return ops.sgm_disparity(torch.from_numpy(im).cuda(), torch.from_numpy(pat).cuda(), ndisp=shape[3], **PARAMS[pi], **kw)


@pytest.mark.parametrize('kind', INPUTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_every_stage_equals_the_reference(shape, kind):
    for pi in range(len(PARAMS)):
        ref = _ref(shape, kind, pi)
        disp, dbg = _run(shape, kind, pi, want_debug=True)
        torch.cuda.synchronize()
        assert disp.shape == (shape[0], shape[1], shape[2]) and disp.dtype == torch.float32
        assert dbg['census'].dtype == torch.int64 and dbg['vol'].dtype == torch.int16 and dbg['d_int'].dtype == torch.int32
        assert torch.equal(dbg['census'].cpu(), torch.from_numpy(ref['census'])), (pi, 'census')
        assert torch.equal(dbg['vol'].cpu(), torch.from_numpy(ref['vol'])), (pi, 'vol')
        assert torch.equal(dbg['d_int'].cpu(), torch.from_numpy(ref['d_int'])), (pi, 'd_int')
        got = disp.cpu()
        assert torch.equal(got != 0, torch.from_numpy(ref['valid'])), (pi, 'valid')
        assert torch.equal(got, torch.from_numpy(ref['disp'])), (pi, 'disp')
    if kind == 'synth':
        assert ref['valid'].any() and not ref['valid'].all()       # both branches of the validity test were taken


def test_repeatable_and_independent_of_the_debug_outputs():
    shape = SHAPES[0]
    a, dbg = _run(shape, 'synth', 0, want_debug=True)
    b, dbg2 = _run(shape, 'synth', 0, want_debug=True)
    c = _run(shape, 'synth', 0)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device='cuda')
    d = _run(shape, 'synth', 0, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and all(torch.equal(dbg[k], dbg2[k]) for k in dbg)
    assert torch.equal(a, c) and torch.equal(a, d)
    assert torch.equal(a.cpu(), torch.from_numpy(_ref(shape, 'synth', 0)['disp']))
    # (n, 1, H, W) in, the same shape out
    from depthinspace_amd import ops
    im, pat = _input(shape, 'synth')
    e = ops.sgm_disparity(torch.from_numpy(im).cuda()[:, None], torch.from_numpy(pat).cuda())
    assert e.shape == (shape[0], 1, shape[1], shape[2]) and torch.equal(e[:, 0], a)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3]], ids=['d64', 'd256'])
def test_graph_capture_on_a_side_stream(shape):
    from depthinspace_amd import ops, lib
    im, pat = _input(shape, 'synth')
    n, H, W, D = shape
    eager = _run(shape, 'synth', 0)
    im_d, pat_d = torch.zeros(n, H, W, device='cuda'), torch.from_numpy(pat).cuda()
    ws = torch.empty(lib.fn('dis_sgm_workspace')(n, H, W, D), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, stream=side):
        out = ops.sgm_disparity(im_d, pat_d, ndisp=D, workspace=ws)
    im_d.copy_(torch.from_numpy(im))                # the capture executed nothing: the replay sees the frames
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    ws.fill_(0xff)                                   # the workspace needs no initialisation and carries nothing between calls
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, eager) and torch.equal(out, eager)


def test_unsupported_arguments_are_refused_before_any_launch():
    from depthinspace_amd import ops, lib
    im = torch.zeros(1, 16, 70, device='cuda')
    pat = torch.zeros(16, 70, device='cuda')
    for kw in (dict(ndisp=96), dict(p2=128), dict(p1=60, p2=60), dict(p1=61, p2=60), dict(p1=0), dict(uniq=100), dict(lr=-1)):
        with pytest.raises(lib.DisHipError):
            ops.sgm_disparity(im, pat, **kw)
    # and by the entry point itself (the python wrapper checks first): a sentinel output stays untouched
    ws = torch.empty(lib.fn('dis_sgm_workspace')(1, 16, 70, 64), dtype=torch.uint8, device='cuda')
    out = torch.full((1, 16, 70), -7.0, device='cuda')
    for nd, p1, p2 in ((96, 7, 60), (64, 7, 128), (64, 60, 60)):
        with pytest.raises(lib.DisHipError):
            lib.call('dis_sgm_disparity', im, pat, out, None, None, None, 1, 16, 70, nd, p1, p2, 5, 1, ws)
    with pytest.raises(lib.DisHipError):
        lib.call('dis_sgm_disparity', im, pat, out, None, None, None, 1, 16, 70, 64, 7, 60, 5, 1, ws[1:])   # misaligned workspace
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.fn('dis_sgm_workspace')(1, 16, 70, 96) == -1 and lib.fn('dis_sgm_workspace')(1, 9000, 70, 64) == -1
