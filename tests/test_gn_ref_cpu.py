"""tests/gn_ref.py proved without a GPU: its fp64 statements against torch.autograd, the coefficient form against the direct form,
every input generator against the condition its name claims, every row of the shape table against what it claims to reach (grids
and loop trip counts recomputed from the entry points' formulae), the chain length the reduction bar rests on, and the kink
exclusion of the end-to-end test on the fp64 reference alone."""
import pytest
import torch
import torch.nn.functional as F

from tests import gn_ref as G

F64 = torch.float64
EPS32 = float(torch.tensor(G.EPS, dtype=torch.float32))   # the eps the kernels see


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------------- statements
@pytest.mark.parametrize('act,res', [(0, False), (1, True), (1, False), (2, True)])
@pytest.mark.parametrize('case', ['randn', 'offset30', 'outlier_pixel', 'selu_edges'])   # (not cancelling_g: fp64 itself cancels there)
@pytest.mark.parametrize('tag', ['old', 'one_past', 'odd_cg'])
def test_apply_and_bwd_equal_autograd(tag, case, act, res):
    """apply + bwd in fp64 with the raw moments are GroupNorm(1 group) (+ residual, + SELU / ReLU) and its gradients"""
    d = G.inputs(case, tag)
    assert float(G.moments(d['st'], d['x'][0].numel(), G.EPS).var_raw.min()) > 0.5   # var well above 0
    x, ga, be, r = [d[k].double().requires_grad_(True) for k in ('x', 'gamma', 'beta', 'res')]
    y = F.group_norm(x.permute(0, 2, 1), 1, ga, be, eps=EPS32).permute(0, 2, 1)
    if res:
        y = y + r
    y = F.selu(y) if act == 1 else (F.relu(y) if act == 2 else y)
    y.backward(d['gy'].double())
    yr = G.apply(d['x'], d['st'], d['gamma'], d['beta'], d['res'] if res else None, act, raw=True)
    assert _rel(yr, y.detach()) < 1e-12
    b = G.bwd(d['gy'], yr, d['x'], d['st'], d['gamma'], act, 0, raw=True)
    assert _rel(b['gx'], x.grad) < 1e-12
    assert _rel(b['grad_gamma'], ga.grad) < 1e-12 and _rel(b['grad_beta'], be.grad) < 1e-12
    if res:
        assert _rel(b['gres'], r.grad) < 1e-12


def test_in_act_is_the_chain_rule_through_a_selu_producer():
    """in_act: x is a SELU output and gx the gradient wrt the producer's pre-activation value"""
    d = G.inputs('randn', 'old')
    pre = d['x'].double().requires_grad_(True)
    xs = F.selu(pre)
    y = F.group_norm(xs.permute(0, 2, 1), 1, d['gamma'].double(), d['beta'].double(), eps=EPS32).permute(0, 2, 1)
    y.backward(d['gy'].double())
    st = G.stats(xs.detach())[0]
    b = G.bwd(d['gy'], None, xs.detach(), st, d['gamma'], 0, 1, raw=True)
    assert _rel(b['gx'], pre.grad) < 1e-12


@pytest.mark.parametrize('in_act', [0, 1])
@pytest.mark.parametrize('case', ['randn', 'offset30'])
@pytest.mark.parametrize('tag', ['old', 'one_past', 'one_vec'])
def test_coef_form_equals_direct_form(tag, case, in_act):
    d = G.inputs(case, tag)
    m = d['x'][0].numel()
    b = G.bwd(d['gy'], None, d['x'], d['st'], d['gamma'], 0, in_act)
    A, B, _, _ = G.sums(d['gy'], d['x'])
    k = G.coef(A, B, d['st'], d['gamma'], m)
    gx = G.apply_coef(d['gy'], d['x'], k['k1'], k['kx'], k['k0'], in_act)
    assert float((gx - b['gx']).abs().max()) < 1e-10 * float(b['gx'].abs().max())
    assert _rel(k['grad_gamma'], b['grad_gamma']) < 1e-10 and _rel(k['grad_beta'], b['grad_beta']) < 1e-10


def test_act_grad_from_out_is_the_derivative():
    v = torch.linspace(-6, 6, 4001, dtype=F64).requires_grad_(True)
    for act, f in ((1, F.selu), (2, F.relu)):
        y = f(v)
        (gr,) = torch.autograd.grad(y.sum(), v)
        assert float((G.act_grad_from_out(y.detach(), act, raw=True) - gr).abs().max()) < 1e-14
        assert float((G.act_apply(v.detach(), act, raw=True) - y.detach()).abs().max()) < 1e-14


def test_yardstick_is_the_same_lines_in_fp32():
    d = G.inputs('randn', 'old')
    y32 = G.apply(d['x'], d['st'], d['gamma'], d['beta'], d['res'], 1, dtype=torch.float32)
    b32 = G.bwd(d['gy'], y32, d['x'], d['st'], d['gamma'], 1, 0, dtype=torch.float32)
    assert y32.dtype == torch.float32 and all(v.dtype == torch.float32 for v in b32.values())
    y64 = G.apply(d['x'], d['st'], d['gamma'], d['beta'], d['res'], 1)
    assert 0 < _rel(y32.double(), y64) < 2e-6


# ---------------------------------------------------------------------------------------------------------------- generators
@pytest.mark.parametrize('tag', list(G.SHAPES))
def test_generators_meet_their_names(tag):
    n, hw, c = G.SHAPES[tag]
    m = hw * c
    for case, R in G.OFFSET_R.items():
        x = G.inputs(case, tag)['x'].double()
        ratio = x.mean(dim=(1, 2)) / x.std(dim=(1, 2), unbiased=False)
        assert bool(((ratio / R - 1).abs() < 0.1).all()), (case, ratio)
    d = G.inputs('constant_sample', tag)
    x0 = d['x'][0].double()
    v = float((x0 * x0).sum() / m - (x0.sum() / m) ** 2)
    assert v <= 0 or v < 1e-12, v
    assert float(G.moments(d['st'], m, G.EPS).var_raw[0]) < 1e-12
    if n > 1:
        d = G.inputs('tiny_sample', tag)
        assert float(G.moments(d['st'], m, G.EPS).var_raw[1]) < G.EPS / 100
        assert float(d['gy'][1].abs().max()) < 1e-5
    d = G.inputs('outlier_pixel', tag)
    assert bool((d['x'][0, hw // 2] == 1e4).all()) and float(d['gy'][1 % n].max()) == 1e4
    d = G.inputs('selu_edges', tag)
    la = G.selu_lambda_alpha_f32()
    for t in (d['x'], d['y_edges']):
        assert float(t.min()) >= -la
        if t.numel() >= 8:
            assert bool((t == -la).any()) and bool((t == 2.0 ** -149).any()) and bool((t == 0).any())
            assert bool(((t == 0) & torch.signbit(t)).any())


@pytest.mark.parametrize('tag', G.BWD_TAGS)
def test_cancelling_g_cancels(tag):
    """max |gx| / max |g rstd gamma| < 1e-6 away from the patches, in fp64 (and the patches themselves are O(1))"""
    n, hw, c = G.SHAPES[tag]
    d = G.inputs('cancelling_g', tag)
    b = G.bwd(d['gy'], None, d['x'], d['st'], d['gamma'], 0, 0)
    mo = G.moments(d['st'], hw * c, G.EPS)
    big = d['gy'].double() * mo.rstd.view(n, 1, 1) * d['gamma'].double()
    away = G.away_mask(n, hw, c)
    if hw == 1:   # one pixel: no patch, everything cancels
        assert float(b['gx'].abs().max()) / float(big.abs().max()) < 1e-6
        return
    assert bool(away.any())
    assert float(b['gx'][away].abs().max()) / float(big[away].abs().max()) < 1e-6
    assert float(b['gx'][~away].abs().max()) > 0.1 * float(mo.rstd.min())   # the patches are there, O(1) in dL/dxhat


# ---------------------------------------------------------------------------------------------------------------- shapes
def test_shape_table_reaches_what_it_claims():
    S = lambda tag: G.SHAPES[tag]
    geo = lambda k, tag, slots=None: G.geometry(k, *S(tag), slots)
    assert S('one_vec')[1] * S('one_vec')[2] == 4
    g = geo('dis_gn_stats', 'one_round')
    assert g['grid'] == 1 and g['rounds'] == 1 and not g['guarded_tail']
    g = geo('dis_gn_stats', 'one_past')
    assert g['grid'] == 2 and g['rounds'] == 1 and g['guarded_tail']
    n, hw, c = S('odd_cg')
    assert c // 4 == 3 and 256 % (c // 4) != 0 and 'odd_cg' not in G.BWD_TAGS
    assert S('maxc')[2] == G.GN_MAXC
    for tag, cap in (('cap256', 256), ('cap64', 64), ('cap32', 32)):
        g = geo('dis_gn_stats', tag)
        assert g['cap'] == cap and g['capped'] and g['grid'] == cap and g['rounds'] > 1 and g['guarded_tail'], (tag, g)
    g = geo('dis_gn_apply', 'cap256')
    assert g['capped'] and g['grid'] == 512 and g['trips'] > 1
    assert geo('dis_gn_bwd_res_sums', 'cap64', G.SLOTS_FULL)['items'] > 1
    g = geo('dis_gn_apply_bwd', 'cap32')
    assert g['nred'] == 64 and g['unrolled'] and g['tail'] and S('cap32')[0] == 16
    g = geo('dis_gn_apply_bwd', 'one_sample_big')
    assert g['nred'] == 512 and g['unrolled'] and g['apply_trips'] > 1
    assert geo('dis_gn_bwd_apply_coef', 'cap32')['trips'] >= 1 and geo('dis_gn_apply', 'one_sample_big')['trips'] > 1
    g = geo('dis_gn_apply_bwd', 'old')       # what the old test never reached
    assert not g['unrolled'] and geo('dis_gn_stats', 'old')['rounds'] == 1 and geo('dis_gn_apply', 'old')['trips'] == 1
    assert set(G.SUMS_TAGS) == {t for t in G.SHAPES if S(t)[2] in (4, 8, 16, 32)}
    assert set(G.E2E_TAGS) <= set(G.BWD_TAGS)
    # the slot summation: no round / rounds and tail / a tail behind whole rounds
    c1 = G.geometry('dis_gn_bwd_coef', 1, 1, 4, 240)
    assert c1['rounds'] == 0 and c1['tail'] == 15
    assert [G.geometry('dis_gn_bwd_coef', 1, 1, 4, s)['rounds'] for s in G.COEF_SLOTS] == [0, 0, 0, 0, 1, 1, 1, 2, 2]
    assert G.geometry('dis_gn_bwd_coef', 1, 1, 4, 257)['tail'] == 1 and G.geometry('dis_gn_bwd_coef', 1, 1, 4, 256)['tail'] == 0
    # the activation kernels: the largest count / pixel count makes every block loop
    assert G.geometry('dis_act_bwd', 1, G.ACT_COUNTS[-1], 4)['trips'] == 2
    for c in G.ACT_LD_C:
        if 256 % (c // 4) == 0:
            g = G.geometry('dis_act_bwd_ld_bias', 1, G.act_ld_npix(c)[-1], c)
            assert g['blocks'] == 1024 and g['items'] == 2


def test_chain_length_holds_the_reduction_bar():
    """SUM_BAR rests on: no thread chains more than MAX_CHAIN fp32 additions at any shape of any table"""
    assert (G.MAX_CHAIN + 3) * G.U32 < G.SUM_BAR
    for tag, (n, hw, c) in G.SHAPES.items():
        assert G.chain_length('dis_gn_stats', n, hw, c) <= G.MAX_CHAIN, tag
        if tag in G.BWD_TAGS:
            assert G.chain_length('dis_gn_apply_bwd', n, hw, c) <= G.MAX_CHAIN, tag
    rows = G.res_sums_table()
    assert {t for t, s in rows if s == G.SLOTS_FULL} == set(G.SUMS_TAGS) and {s for _, s in rows} == {1, 8, G.SLOTS_FULL}
    for tag, slots in rows:
        assert G.chain_length('dis_gn_bwd_res_sums', *G.SHAPES[tag], slots) <= G.MAX_CHAIN, (tag, slots)
    for c in G.ACT_LD_C:
        if 256 % (c // 4) == 0:
            for npix in G.act_ld_npix(c):
                assert G.chain_length('dis_act_bwd_ld_bias', 1, npix, c) <= G.MAX_CHAIN, (c, npix)
    for slots in G.COEF_SLOTS:
        assert G.chain_length('dis_gn_bwd_coef', 1, G.COEF_HW, 4, slots) == 0   # fp64 throughout


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('act,res', [(0, False), (1, True), (1, False)])
@pytest.mark.parametrize('case', ['randn', 'offset30'])
@pytest.mark.parametrize('tag', G.E2E_TAGS)
def test_kink_exclusion_stays_under_its_cap(tag, case, act, res):
    d = G.inputs(case, tag)
    pre = G.apply(d['x'], d['st'], d['gamma'], d['beta'], d['res'] if res else None, act, raw=True, pre=True)
    share = G.excluded_share(G.kink_keep(pre, act))
    assert share <= G.EXCLUDE_CAP, share
    assert share <= 1e-3   # (about 1e-5 with these generators)


def test_checks_hold_the_bar_rule():
    ref = torch.tensor([1.0, -2.0, 0.5], dtype=F64)
    yard = ref + torch.tensor([0.0, 1e-6, 0.0], dtype=F64)           # yardstick 5e-7 of the largest entry away: bar 2e-6
    assert G.check(ref + 3.9e-6, ref, yard, 1e-7) == pytest.approx(3.9e-6 / 2 / 2e-6)
    with pytest.raises(AssertionError):
        G.check(ref + 4.1e-6, ref, yard, 1e-7)
    with pytest.raises(AssertionError):
        G.check(ref + 4.1e-6, ref, ref, 2e-6)                         # an exact yardstick: (a) alone
    G.check(ref + 4.1e-6, ref, ref, 2e-6, extra=1e-7)
    with pytest.raises(AssertionError):
        G.check(torch.tensor([float('nan'), -2.0, 0.5]), ref, yard, 1.0)
    G.check_sum(ref + 0.9e-6, ref, torch.ones(3, dtype=F64))
    with pytest.raises(AssertionError):
        G.check_sum(ref + 1.1e-6, ref, torch.ones(3, dtype=F64))
