"""CPU: tests/conv3d_ref.py, the float64 reference of tests/test_conv3d_fp64_gpu.py, proven against what the REFERENCE module
computed (tests/golden/ops.npz, c3_*), and its generators proven - from the reference alone - to stay inside the kink cap."""
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dis_oracle as O
from tests import conv3d_ref as R

NAME = 'blocks.0.conv3d_1'
GOLDEN_KEYS = {'dense1_w': 'dense1.0.weight', 'dense1_b': 'dense1.0.bias', 'dense2_w': 'dense2.0.weight',
               'dense2_b': 'dense2.0.bias', 'w': 'w'}


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('stride', [1, 2])
def test_reference_reproduces_the_fixture(golden_dir, stride, dtype):
    """conv3d() + F.group_norm on the fixture's inputs, with the oracle's own top-9 ids: forward and every gradient equal what
    the reference module produced, with test_conv3d_golden's bars (2e-5 / 5e-5 / 1e-4 of the largest entry)"""
    G = np.load(os.path.join(golden_dir, 'ops.npz'))
    xyz, feat, mask = [torch.from_numpy(G[k]) for k in ('c3_xyz', 'c3_feat', 'c3_mask')]
    TL, bs, C, h, w = feat.shape
    p = O.init_params({k: v for k, v in O.mf_param_shapes().items() if k.startswith(NAME)}, seed=5)
    with torch.no_grad():
        _, idx, _ = O.conv3d_knn(p, NAME, xyz, feat, mask, stride, TL, return_index=True)
    assert np.array_equal(np.sort(idx.numpy(), -1), G[f'c3_s{stride}_idx_sorted'])
    geom = torch.cat([xyz, mask], dim=2).permute(1, 3, 4, 0, 2).unsqueeze(0).contiguous()   # (1,bs,h,w,slot,4)
    wf = feat.permute(1, 3, 4, 0, 2).unsqueeze(0).contiguous().to(dtype).requires_grad_(True)
    ps = {k: p[f'{NAME}.{v}'].detach().to(dtype).requires_grad_(True) for k, v in GOLDEN_KEYS.items()}
    gamma, beta = [p[f'{NAME}.bn.{k}'].detach().to(dtype).requires_grad_(True) for k in ('weight', 'bias')]
    y, agg, _ = R.conv3d(geom, wf, [ps[k] for k in R.PARAMS], idx.unsqueeze(0).to(torch.uint8), stride, dtype)
    assert y.dtype == dtype and agg.dtype == dtype
    out = F.group_norm(y[0].permute(0, 3, 1, 2), 1, gamma, beta, eps=1e-5)
    out.backward(torch.from_numpy(G[f'c3_s{stride}_go']).to(dtype))
    assert relerr(out, torch.from_numpy(G[f'c3_s{stride}_out'])) < 2e-5
    assert relerr(wf.grad[0].permute(3, 0, 4, 1, 2), torch.from_numpy(G[f'c3_s{stride}_gfeat'])) < 5e-5
    for k, v in GOLDEN_KEYS.items():
        assert relerr(ps[k].grad, torch.from_numpy(G[f'c3_s{stride}_g:{v}'])) < 1e-4, k
    assert relerr(gamma.grad, torch.from_numpy(G[f'c3_s{stride}_g:bn.weight'])) < 1e-4
    assert relerr(beta.grad, torch.from_numpy(G[f'c3_s{stride}_g:bn.bias'])) < 1e-4


def test_reference_states_padding_and_ids_explicitly():
    """one output pixel by hand: 1 x 1 map, every tap but the centre is padding (xyz = 0, features = 0)"""
    g = torch.Generator().manual_seed(3)
    TL = 2
    geom = torch.randn(1, 1, 1, 1, TL, 4, generator=g).double()
    wf = torch.randn(1, 1, 1, 1, TL, 32, generator=g).double()
    params = [q.double() for q in R.make_params(g)]
    ids = [0, 1, 8, 9, 17, 3, 4, 10, 16]   # tap 4 (ids 8, 9) is the centre; the seven others are outside the map
    idx = torch.tensor(ids, dtype=torch.uint8).view(1, 1, 1, 1, 9)
    y, agg, (pre1, pre2, pre_y) = R.conv3d(geom, wf, params, idx, 1, torch.float64)
    w1, b1, w2, b2, wm = params
    ctr = geom[0, 0, 0, 0, 0, :3]
    want = torch.zeros(32, dtype=torch.float64)
    for n, i in enumerate(ids):
        inside = i // TL == 4
        xyz = geom[0, 0, 0, 0, i % TL, :3] if inside else torch.zeros(3, dtype=torch.float64)
        h2 = F.selu(w2 @ F.selu(w1 @ (xyz - ctr) + b1) + b2)
        assert torch.allclose(pre1[0, 0, 0, 0, n], w1 @ (xyz - ctr) + b1, rtol=0, atol=1e-14)
        if inside:
            want += h2 * wf[0, 0, 0, 0, i % TL]
    assert torch.allclose(agg.view(-1), want, rtol=0, atol=1e-13)
    assert torch.allclose(y.view(-1), F.selu(want @ wm), rtol=0, atol=1e-13)


CAP_CASES = [c + ('plain',) for c in R.edge_cases()] + R.range_cases()


def test_every_generator_case_is_inside_the_kink_cap():
    """from the float64 forward alone: every case of the GPU file zeroes at most KINK_CAP of its output pixels and is reached
    within MAX_ADVANCE seed advances; the zeroed pixels are exactly those with a pre-activation inside the margin; few-pixel
    cases do advance"""
    advanced, worst, forward_only = 0, 0.0, []
    for (h, w, bs, tl, stride, ids, rng) in CAP_CASES:
        c = R.make_case(tl, bs, h, w, stride, ids, rng, grads=False)
        if rng not in R.RANGES_WITH_BACKWARD:
            forward_only.append(c.share)
            continue
        assert c.advances <= R.MAX_ADVANCE and c.share <= R.KINK_CAP, (h, w, bs, tl, stride, ids, rng)
        assert c.share == float(c.zeroed.double().mean())
        assert bool((c.gy[c.zeroed] == 0).all()) and bool((c.gy[~c.zeroed] != 0).all())
        advanced += c.advances > 0
        worst = max(worst, c.share)
    print(f'{len(CAP_CASES)} cases, {advanced} advanced their seed, largest zeroed share {worst:.4f}')
    assert worst > 0, 'no case has a pixel inside the margin: the margin is not exercised'
    # why 'outlier' is a forward case: the outlier sets the layer's largest pre-activation, the margin covers most ordinary pixels
    print(f'forward-only cases: share inside the margin {min(forward_only):.2f} ... {max(forward_only):.2f}')
    assert min(forward_only) > 4 * R.KINK_CAP


def test_generation_is_deterministic():
    R.make_case.cache_clear()
    a = R.make_case(2, 5, 1, 1, 1, 'random', 'plain', grads=False)
    R.make_case.cache_clear()
    b = R.make_case(2, 5, 1, 1, 1, 'random', 'plain', grads=False)
    assert a is not b and a.advances == b.advances
    for k in ('geom', 'wf', 'idx', 'gy', 'base'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize('tl', R.TLS)
def test_random_id_sets_are_distinct_and_in_range(tl):
    g = torch.Generator().manual_seed(tl)
    idx = R.random_ids(tl, 3, 7, 5, g)
    assert idx.dtype == torch.uint8 and tuple(idx.shape) == (tl, 3, 7, 5, 9)
    assert int(idx.min()) >= 0 and int(idx.max()) <= 9 * tl - 1
    srt = idx.long().sort(dim=-1).values
    assert bool((srt[..., 1:] > srt[..., :-1]).all()), 'ids of a pixel repeat'
    assert len(torch.unique(idx)) == 9 * tl   # every candidate is drawn somewhere, padded border taps included


def test_select_source_is_the_bit_exact_selection():
    """the 'select' ids of a case are tests/bitexact.py's on the case's own geometry, distinct as well"""
    c = R.make_case(3, 3, 5, 7, 2, 'select', 'plain', grads=False)
    assert torch.equal(c.idx, R.select_ids(c.xyz, c.mask, 2))
    srt = c.idx.long().sort(dim=-1).values
    assert bool((srt[..., 1:] > srt[..., :-1]).all())
