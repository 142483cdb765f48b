"""TEST INFRASTRUCTURE (CPU only): Conv3D (csrc/conv3d_knn.hip; reference model/multi_frame_networks.py:432-512) stated plainly
in torch for given neighbour ids, parameterised by dtype, gradients by autograd - in float64 it is the reference of
tests/test_conv3d_fp64_gpu.py, in float32 the yardstick the bars of that file are scaled with - and the input generators of that
file: geometry, masks, the two id sources, the range cases and the upstream gradient.

THE OPERATOR.  geom (tl,bs,h,w,TL,4) holds xyz + mask of the TL slots of a pixel, wf (tl,bs,h,w,TL,32) their features,
idx (tl,bs,ho,wo,9) the ids of the 9 neighbours of every output pixel, ho = (h - 1) // stride + 1.  Id = tap * TL + slot names
the candidate at (oy * stride - 1 + tap // 3, ox * stride - 1 + tap % 3, slot); outside the map its xyz and features are 0.
    local = xyz - geom[t, b, oy * stride, ox * stride, 0, :3]
    h1 = selu(W1 local + b1),  h2 = selu(W2 h1 + b2),  agg = sum_n h2 * feat,  y = selu(agg @ w)
The mask takes no part: it decides the selection only.

KINKS.  SELU' jumps at 0, so a float32 evaluation whose pre-activation has the other sign than the float64 one has another
gradient.  The upstream gradient is therefore ZERO on every output pixel where a float64 pre-activation (dense1 and dense2 of
its nine neighbours, the output mix) satisfies 0 < |pre| < KINK * max |pre of that layer|: such a pixel contributes nothing to
any gradient, on either side.  KINK = 4e-6 is about 13 x the float32 evaluation's own pre-activation error (3e-7 of the layer's
largest entry with the parameter scales drawn here).  Exact zeros stay: an all-padded pixel has agg == 0 and pre == 0 in every
evaluation, and every evaluation takes SELU's negative branch there.  At most KINK_CAP of a case's output pixels may be zeroed
this way; the generator advances its seed (at most MAX_ADVANCE times) until a case is inside the cap - with two output pixels
a single one is already half the case.  Forward values are compared on every pixel.
"""
import functools
import numpy as np
import torch
import torch.nn.functional as F

from tests import bitexact as B
from tests import pixel_ref as P

F64, F32 = torch.float64, torch.float32
NB, C, H1 = 9, 32, 16
KINK = 4e-6
KINK_CAP = 0.05
MAX_ADVANCE = 8
PARAMS = ('dense1_w', 'dense1_b', 'dense2_w', 'dense2_b', 'w')          # the order of the entry points' arguments
GP_SLICES = {'w': (0, 1024), 'dense1_w': (1024, 1072), 'dense1_b': (1072, 1088), 'dense2_w': (1088, 1600),
             'dense2_b': (1600, 1632)}                                   # the kernels' parameter-gradient block (1632 floats)
PARAM_SHAPES = {'dense1_w': (H1, 3), 'dense1_b': (H1,), 'dense2_w': (C, H1), 'dense2_b': (C,), 'w': (C, C)}
MASK_KINDS = ('holes', 'dead_pixels', 'all_masked')
ID_SOURCES = ('select', 'random')
RANGES = ('plain', 'outlier', 'tiny')
# 'outlier' (one feature row x 1e4) is a forward case: the outlier sets the largest pre-activation of the output mix, so the
# margin KINK * max|pre| spans the ordinary pixels' range and no seed keeps such a case inside KINK_CAP
RANGES_WITH_BACKWARD = ('plain', 'tiny')

# (h, w, bs) of the edge-shape sweep, see the table in tests/test_conv3d_fp64_gpu.py
EDGE_SHAPES = ((1, 1, 1), (1, 1, 5), (1, 7, 2), (7, 1, 2), (2, 2, 1), (3, 3, 1), (5, 7, 3), (13, 9, 2), (6, 8, 2), (12, 14, 2),
               (40, 36, 2))
TLS = (2, 3, 4)
RANGE_SHAPE = (5, 7, 3)


def out_dims(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def conv3d(geom, wf, params, idx, stride, dtype):
    """-> y (tl,bs,ho,wo,32), agg (tl,bs,ho,wo,32), (pre1 (..,9,16), pre2 (..,9,32), pre_y (..,32)), evaluated in `dtype`.
    params = (dense1_w (16,3), dense1_b (16), dense2_w (32,16), dense2_b (32), w (32,32)); differentiable in wf and params."""
    tl, bs, h, w, TL, _ = geom.shape
    ho, wo = out_dims(h, w, stride)
    assert tuple(idx.shape) == (tl, bs, ho, wo, NB) and tuple(wf.shape) == (tl, bs, h, w, TL, C)
    w1, b1, w2, b2, wm = [p.to(dtype) for p in params]
    xyz = geom[..., :3].to(dtype)
    xyz_p = F.pad(xyz, (0, 0, 0, 0, 1, 1, 1, 1))           # zero border of one pixel around the map
    wf_p = F.pad(wf.to(dtype), (0, 0, 0, 0, 1, 1, 1, 1))
    ids = idx.long()
    tap, slot = ids // TL, ids % TL
    py = torch.arange(ho).view(1, 1, ho, 1, 1) * stride + tap // 3          # row in the padded map: (oy s - 1 + tap // 3) + 1
    px = torch.arange(wo).view(1, 1, 1, wo, 1) * stride + tap % 3
    ti = torch.arange(tl).view(tl, 1, 1, 1, 1)
    bi = torch.arange(bs).view(1, bs, 1, 1, 1)
    nb_xyz = xyz_p[ti, bi, py, px, slot]                   # (tl,bs,ho,wo,9,3)
    nb_feat = wf_p[ti, bi, py, px, slot]                   # (tl,bs,ho,wo,9,32)
    ctr = xyz[:, :, ::stride, ::stride, 0]                 # (tl,bs,ho,wo,3)
    local = nb_xyz - ctr.unsqueeze(4)
    pre1 = local @ w1.t() + b1
    pre2 = F.selu(pre1) @ w2.t() + b2
    agg = (F.selu(pre2) * nb_feat).sum(dim=4)
    pre_y = agg @ wm
    return F.selu(pre_y), agg, (pre1, pre2, pre_y)


def kink_pixels(pres):
    """(tl,bs,ho,wo) bool: the output pixels with a pre-activation inside the kink margin (module docstring)"""
    bad = None
    for p in pres:
        a = p.detach().to(F64).abs()
        near = (a > 0) & (a < KINK * float(a.max()))
        near = near.reshape(*near.shape[:4], -1).any(dim=-1)
        bad = near if bad is None else bad | near
    return bad


def run(geom, wf, params, idx, stride, dtype, gy):
    """value and gradients under the upstream gradient gy: {'y', 'agg', 'grad_wf', one entry per PARAMS} in `dtype`"""
    wf_ = wf.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    y, agg, _ = conv3d(geom, wf_, ps, idx, stride, dtype)
    y.backward(gy.to(dtype))
    out = {'y': y.detach(), 'agg': agg.detach(), 'grad_wf': wf_.grad}
    out.update({k: p.grad for k, p in zip(PARAMS, ps)})
    return out


# --------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------
def geometry(tl, bs, h, w, g, mask_kind='holes'):
    """-> xyz (tl,slot,bs,3,h,w), mask (tl,slot,bs,1,h,w) as tests/bitexact.py takes them: z near 3, x / y on the pixel grid,
    noise 0.05 (tests/test_track_length_gpu.py::_conv3d_inputs); 'holes': a fifth of the candidates masked, slot 0 valid;
    'dead_pixels': moreover a quarter of the pixels masked in every slot; 'all_masked': no valid candidate anywhere"""
    xyz = torch.randn(tl, tl, bs, 3, h, w, generator=g) * 0.05
    xyz[:, :, :, 2] += 3.0
    xyz[:, :, :, 0] += (torch.arange(w, dtype=F32).view(1, w) - w / 2) * 0.01
    xyz[:, :, :, 1] += (torch.arange(h, dtype=F32).view(h, 1) - h / 2) * 0.01
    mask = (torch.rand(tl, tl, bs, 1, h, w, generator=g) > 0.2).float()
    mask[:, 0] = 1
    dead = torch.rand(tl, 1, bs, 1, h, w, generator=g) < 0.25
    if mask_kind == 'dead_pixels':
        mask = mask * (~dead).float()
    elif mask_kind == 'all_masked':
        mask = torch.zeros_like(mask)
    else:
        assert mask_kind == 'holes'
    return xyz, mask


def to_geom(xyz, mask):
    """(tl,slot,bs,3|1,h,w) -> the kernels' (tl,bs,h,w,slot,4)"""
    return torch.cat([xyz, mask], dim=3).permute(0, 2, 4, 5, 1, 3).contiguous()


def select_ids(xyz, mask, stride):
    """the selection of tests/bitexact.py: ids (tl,bs,ho,wo,9) uint8 in torch.topk's order"""
    return torch.from_numpy(B.conv3d_select(xyz.numpy(), mask.numpy(), stride).astype(np.uint8))


def random_ids(tl, bs, ho, wo, g):
    """for every output pixel the first 9 of a random permutation of the 9 TL candidates: DISTINCT, as every selection is and
    as the class-ordered backward relies on (one add per gradient row and class launch)"""
    return torch.rand(tl, bs, ho, wo, NB * tl, generator=g).argsort(dim=-1)[..., :NB].to(torch.uint8).contiguous()


def make_params(g):
    """weights U(+-s / sqrt(fan_in)) with a scale s in [1.0, 1.6] per tensor, biases 0.1 U(-1, 1)"""
    out = []
    for k in PARAMS:
        shp = PARAM_SHAPES[k]
        u = torch.rand(shp, generator=g) * 2 - 1
        if len(shp) == 1:
            out.append(0.1 * u)
        else:
            s = 1.0 + 0.6 * float(torch.rand((), generator=g))
            out.append(u * (s / shp[1] ** 0.5))
    return tuple(out)


class Case(object):
    """inputs of one comparison and what the reference alone says about them"""
    pass


def _inputs(tl, bs, h, w, stride, ids, rng, attempt):
    g = P._gen(tl, bs, h, w, stride, ID_SOURCES.index(ids), RANGES.index(rng), attempt)
    c = Case()
    c.tl, c.bs, c.h, c.w, c.stride, c.ids, c.rng, c.advances = tl, bs, h, w, stride, ids, rng, attempt
    c.ho, c.wo = out_dims(h, w, stride)
    xyz, mask = geometry(tl, bs, h, w, g)
    if rng == 'tiny':
        xyz = xyz * 100.0
    c.xyz, c.mask = xyz, mask
    c.geom = to_geom(xyz, mask)
    c.wf = torch.randn(tl, bs, h, w, tl, C, generator=g)
    c.params = make_params(g)
    c.idx = select_ids(xyz, mask, stride) if ids == 'select' else random_ids(tl, bs, c.ho, c.wo, g)
    if rng == 'tiny':
        c.wf = c.wf * 1e-6
    elif rng == 'outlier':   # the first in-map candidate of the middle output pixel of (target 0, sample 0): a row that is read
        oy, ox = c.ho // 2, c.wo // 2
        for n in range(NB):
            i = int(c.idx[0, 0, oy, ox, n])
            iy, ix = oy * stride - 1 + (i // tl) // 3, ox * stride - 1 + (i // tl) % 3
            if 0 <= iy < h and 0 <= ix < w:
                c.wf[0, 0, iy, ix, i % tl] *= 1e4
                break
        else:
            raise AssertionError('no in-map candidate')
    c.gy = torch.randn(tl, bs, c.ho, c.wo, C, generator=g)
    c.base = torch.randn(tl, bs, h, w, tl, C, generator=g)
    return c


def kink_share(c):
    """share of the case's output pixels inside the kink margin, from the float64 forward alone; sets c.zeroed"""
    with torch.no_grad():
        _, _, pres = conv3d(c.geom, c.wf, c.params, c.idx, c.stride, F64)
    c.zeroed = kink_pixels(pres)
    return float(c.zeroed.to(F64).mean())


@functools.lru_cache(maxsize=4)
def make_case(tl, bs, h, w, stride, ids, rng='plain', grads=True):
    """The case of these arguments: the first seed advance whose kink share is inside KINK_CAP (seed 0 for a range outside
    RANGES_WITH_BACKWARD); c.gy is zero on c.zeroed.  With `grads`, c.ref / c.f32 hold run() in float64 / float32.  The result
    is shared: treat it as read-only."""
    for attempt in range(MAX_ADVANCE + 1):
        c = _inputs(tl, bs, h, w, stride, ids, rng, attempt)
        c.share = kink_share(c)
        if c.share <= KINK_CAP or rng not in RANGES_WITH_BACKWARD:   # (a forward case: its gradients are not compared)
            break
    else:
        raise AssertionError(f'no seed within {MAX_ADVANCE} advances keeps {(tl, bs, h, w, stride, ids, rng)} inside the cap')
    c.gy = c.gy * (~c.zeroed).unsqueeze(-1).float()
    if grads:
        c.ref = run(c.geom, c.wf, c.params, c.idx, c.stride, F64, c.gy)
        c.f32 = run(c.geom, c.wf, c.params, c.idx, c.stride, F32, c.gy)
    return c


def edge_cases():
    """(h, w, bs, tl, stride, ids) of the edge-shape sweep"""
    return [(h, w, bs, tl, s, ids) for (h, w, bs) in EDGE_SHAPES for tl in TLS for s in (1, 2) for ids in ID_SOURCES]


def range_cases():
    h, w, bs = RANGE_SHAPE
    return [(h, w, bs, tl, s, ids, rng) for tl in TLS for s in (1, 2) for ids in ID_SOURCES for rng in RANGES[1:]]
