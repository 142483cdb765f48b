"""The small kernels around the resizes in csrc/layout_ops.hip, all compared for equality.

  * dis_pack4_nhwc_strided through ops.pack4_nhwc in the three forms the networks use (the two planes of an (N,2,H,W) tensor
    through a stride of 2 HW and an offset view plus two more sources; one source and three zero channels; the C planes of one
    flat tensor), and dis_pack4_nhwc with a NULL source, against torch.stack.  (2,513,512) has 2048 x 256 + 1024 pixels: a
    second trip of the grid-stride loop.
  * dis_slot_weights and dis_mask_weight_slots against numpy fp32 written in the kernels' order,
        mean = fl(fl(sum_k m_k) / tl)       wgt = fl(m / mean)       out = fl(fl(v m) / mean)      [+ old: fl(out + old)]
    (the masks are 0 / 1, so the sum is exact; IEEE division is correctly rounded on the device as on the host - tests/bitexact.py's
    disp_to_depth relies on the same - so equality is the bar).  tl = 3 gives the means fl(1/3) and fl(2/3), which are not exact.
    The accumulate=1 form - the backward of a tensor with a second consumer - is called directly into an output that holds
    known values, and through ops.GradJoin; the autograd backward is the same formula applied to the incoming gradient.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = np.float32
CAP = 2048 * 256
PACK_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 17, 19), (2, 513, 512)]


def _eq(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = torch.nonzero(~(got == want))
        raise AssertionError(f'{what}: {len(bad)} of {got.numel()} elements differ, first at {tuple(int(v) for v in bad[0])} of {tuple(got.shape)}')


@pytest.mark.parametrize('n,h,w', PACK_SHAPES)
def test_pack4_nhwc_forms(n, h, w):
    from depthinspace_amd import ops, lib
    g = torch.Generator().manual_seed(n * 1000 + h)
    hw = h * w
    ir = torch.randn(n, 2, h, w, generator=g)
    amb, d = torch.randn(n, 1, h, w, generator=g), torch.randn(n, 1, h, w, generator=g)
    zero = torch.zeros(n, h, w)
    ird, ambd, dd = ir.cuda(), amb.cuda(), d.cuda()
    # the multi-frame network's input: (ir plane 0, ir plane 1, ambient, disparity)
    got = ops.pack4_nhwc([(ird, 2 * hw), (ird.view(-1)[hw:], 2 * hw), (ambd, hw), (dd, hw)], n, h, w)
    want = torch.stack([ir[:, 0], ir[:, 1], amb[:, 0], d[:, 0]], -1)
    _eq(got, want, 'four sources, two of them planes of one tensor')
    out = torch.full((n, h, w, 4), float('nan'), device='cuda')     # (the same launch into an output that holds NaN)
    lib.call('dis_pack4_nhwc_strided', ird, 2 * hw, ird.view(-1)[hw:], 2 * hw, ambd, hw, dd, hw, out, n, h, w)
    _eq(out, want, 'dis_pack4_nhwc_strided into NaN')
    # one source, the other channels 0.0 (and not -0.0, not NaN)
    got = ops.pack4_nhwc([(ambd, hw)], n, h, w)
    _eq(got, torch.stack([amb[:, 0], zero, zero, zero], -1), 'one source')
    assert not torch.signbit(got[..., 1:]).any()
    # the C planes of one flat tensor (the single-frame network's input), C = 1 .. 4
    for C in (1, 2, 3, 4):
        x = torch.randn(n, C, h, w, generator=g)
        flat = x.cuda().view(-1)
        got = ops.pack4_nhwc([(flat[c * hw:], C * hw) for c in range(C)], n, h, w)
        _eq(got, torch.stack([x[:, c] for c in range(C)] + [zero] * (4 - C), -1), f'{C} planes of one flat tensor')
    # the contiguous entry point, one source NULL, into a NaN-filled output
    s = [torch.randn(n, h, w, generator=g) for _ in range(3)]
    sd = [t.cuda() for t in s]
    for hole in range(4):
        srcs, devs = list(s), list(sd)
        srcs.insert(hole, zero)
        devs.insert(hole, None)
        out = torch.full((n, h, w, 4), float('nan'), device='cuda')
        lib.call('dis_pack4_nhwc', *devs, out, n, h, w)
        _eq(out, torch.stack(srcs, -1), f'dis_pack4_nhwc, source {hole} NULL')
    if (n, h, w) == PACK_SHAPES[-1]:
        assert n * hw > CAP


def _geom(tl, bs, h, w, rng):
    """(tl,bs,h,w,slot,4): random xyz, 0/1 masks with holes, slot 0 all ones"""
    geom = rng.standard_normal((tl, bs, h, w, tl, 4)).astype(f32)
    geom[..., 3] = (rng.random((tl, bs, h, w, tl)) > 0.35).astype(f32)
    geom[..., 0, 3] = 1
    return geom


def _mean(mask):
    """mask (..., tl) -> fl(fl(sum) / tl), summed in slot order"""
    tl = mask.shape[-1]
    msum = np.zeros(mask.shape[:-1], f32)
    for k in range(tl):
        msum = (msum + mask[..., k]).astype(f32)
    return (msum / f32(tl)).astype(f32)


def _weighted(v, mask):
    """v (..., tl, c), mask (..., tl) -> fl(fl(v m) / mean)"""
    return ((v * mask[..., None]).astype(f32) / _mean(mask)[..., None, None]).astype(f32)


SLOT_CASES = [(tl, 2, 5, 7) for tl in (2, 3, 4)] + [(3, 1, 1, 1)]


@pytest.mark.parametrize('tl,bs,h,w', SLOT_CASES + [(2, 1, 513, 512)])
def test_slot_weights(tl, bs, h, w):
    """(2,1,513,512): more pixels than 2048 x 256 threads"""
    from depthinspace_amd import ops, lib
    rng = np.random.default_rng(tl * 100 + h)
    geom = _geom(tl, bs, h, w, rng)
    mask = geom[..., 3]
    assert (mask == 0).any() or h == 1
    if h > 500:
        assert tl * bs * h * w > CAP
    want = (mask / _mean(mask)[..., None]).astype(f32).reshape(tl * bs, h, w, tl)
    gd = torch.from_numpy(geom).cuda()
    out = torch.full((tl * bs, h, w, tl), float('nan'), device='cuda')
    lib.call('dis_slot_weights', gd, out, tl * bs * h * w, tl)
    _eq(out, torch.from_numpy(want), 'dis_slot_weights into NaN')
    _eq(ops.slot_weights(gd), torch.from_numpy(want), 'ops.slot_weights')


@pytest.mark.parametrize('tl,bs,h,w,c', [s + (c,) for s in SLOT_CASES for c in (4, 32)] + [(4, 1, 65, 64, 32)])
def test_mask_weight_slots_forward_accumulate_and_backward(tl, bs, h, w, c):
    """(4,1,65,64) at c = 32: 16640 x 4 x 8 work items, more than 2048 x 256"""
    from depthinspace_amd import ops, lib
    rng = np.random.default_rng(tl * 100 + h + c)
    geom = _geom(tl, bs, h, w, rng)
    mask = geom[..., 3]
    if h > 60:
        assert tl * bs * h * w * tl * (c // 4) > CAP
    v = rng.standard_normal((tl, bs, h, w, tl, c)).astype(f32)
    go = rng.standard_normal(v.shape).astype(f32)
    old = rng.standard_normal(v.shape).astype(f32)
    gd = torch.from_numpy(geom).cuda()
    vd = torch.from_numpy(v).cuda().requires_grad_(True)
    out = ops.mask_weight_slots(vd, gd)
    _eq(out.detach(), torch.from_numpy(_weighted(v, mask)), 'mask_weight_slots forward')
    out.backward(torch.from_numpy(go).cuda())
    _eq(vd.grad, torch.from_numpy(_weighted(go, mask)), 'mask_weight_slots backward')
    # accumulate=1, directly: out = fl(fl(fl(v m) / mean) + old)
    acc = torch.from_numpy(old).cuda()
    lib.call('dis_mask_weight_slots', torch.from_numpy(go).cuda(), gd, acc, tl * bs * h * w, tl, c, 1)
    want_acc = (_weighted(go, mask) + old).astype(f32)
    _eq(acc, torch.from_numpy(want_acc), 'dis_mask_weight_slots accumulate=1')
    # ... and as the networks reach it: the other consumer of the tensor has left its gradient in the GradJoin
    join = ops.GradJoin()
    v2 = torch.from_numpy(v).cuda().requires_grad_(True)
    out2 = ops.mask_weight_slots(v2, gd, join)
    join.first(torch.from_numpy(old).cuda())
    out2.backward(torch.from_numpy(go).cuda())
    _eq(v2.grad, torch.from_numpy(want_acc), 'mask_weight_slots backward into a GradJoin')
    # accumulate=0 overwrites whatever the output held
    fresh = torch.full(v.shape, float('nan'), device='cuda')
    lib.call('dis_mask_weight_slots', torch.from_numpy(v).cuda(), gd, fresh, tl * bs * h * w, tl, c, 0)
    _eq(fresh, torch.from_numpy(_weighted(v, mask)), 'dis_mask_weight_slots accumulate=0 into NaN')
