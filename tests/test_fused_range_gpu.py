"""The fused two-term fp16 ("f16x2": every fp32 operand held as two fp16 terms, one power-of-two scale per staged tile) conv launches
against an fp64 restatement of the SAME composite operation, on inputs built to attack the scale each launch picks for itself:

  dis_conv2d_bwd_fused_f16x2        gy halo per tile (formed gpre in the GroupNorm-backward forms), x or GroupNorm(x) per tile, one
                                    dW exponent per workgroup (FB_SMARGIN bits of headroom, leave-and-restart when a tile is larger)
  dis_conv2d_dgrad_f16x2_gnb        gpre = GroupNorm backward (x SELU') formed on load, split per tile
  dis_conv2d_fwd_bf16x3_gn          GroupNorm(x) formed on load (ops.conv2d_gn_in), dis_conv2d_fwd_f16x2_gnres SELU(GroupNorm(x2) + res)
  dis_conv2d_wgrad_k4s2_f16x2_gnb   gpre formed on load for the 4 x 4 stride-2 weight gradient

Yardstick: the three-term bf16 kernels (8 exponent bits, no scaling) run the unfused composition on the same inputs; bar for every
per-element metric: f16x2 error < 4 x the bf16x3 error + 2e-7 of the normalising magnitude, measured globally, per sample and per
region.  Two fp64 references:
  fp64      the composite operation in double from the fp32 inputs (GroupNorm backward from the per-sample sums, GroupNorm on load);
  operand   the conv / reduction in double of the operand the kernels FORM in fp32 (the stored gpre / block output, bit-identical
            between the fused and the unfused launches; GroupNorm(x) as dis_gn_apply forms it).  Where the elementwise stage cancels
            (cancelling_gpre, tiny_tiles of the GroupNorm-backward forms, offset_gn_input) its fp32 rounding is comparable to the
            small result itself, identical in both kernels - only this reference can see what the SPLIT did there.
The fixed bars of tests/test_bwd_fused_gpu.py (grad_w / grad_b, channel sums within 1e-6 of the largest entry) hold against the
operand reference.

Cases (each names the scale decision it attacks):
  randn            control
  outlier_pixel    one 1e4 pixel in x and one in g, different samples: the tile scale is the outlier's
  tiny_sample      sample 1 scaled by 1e-6: judged against that sample's own largest entry
  tiny_tiles       a 32 x 32 corner of the conv operand at 1e-6 (g and x; in the GroupNorm-backward forms gpre, formed from O(1) g
                   by the GroupNorm backward's own means): all-tiny tiles against their own largest entry, tiles whose halo reaches the
                   O(1) region on absolute error (test_conv_f16x2_dynamic_range's metric)
  cancelling_gpre  g = (alpha + beta xhat) / gamma_c outside a few O(1) patches: the GroupNorm backward cancels to a gpre 1e-9 .. 1e-8
                   of g away from them (printed; asserted < 1e-7) - a tile scale taken from g instead of gpre loses that tile's
                   relative accuracy
  offset_gn_input  x = 1000 + z, GroupNorm gain ~2^-20: formed values ~3e-6 with ~14 significant bits while the raw ones are 1e3 - a
                   scale sized from raw x leaves them 4 - 10 bits.  (A small gain is what makes it visible: the formed values carry
                   the fp32 grid of x * rstd gamma, and a raw-x scale only drops bits below that grid when rstd gamma < ~2^-10.
                   Behind an output SELU - conv2d_gn_in with act = 1, the gnres launch - the SELU's own fp32 rounding of such small
                   outputs, the same in both kernels, dominates: there the case checks the range, the scale decision is seen at act = 0.)
  tiny_gn_output   GroupNorm shift cancels the input of one 32 x 32 corner: normalised ~1e-6 there while the raw input is O(1) (the
                   tiny values carry 2 bits, held by any scale: a check of that tile and the statistics, not of the scale choice)
  exponent_ramp    x and gy scaled per 16 x 16 tile by 2^(7 r), r in {0 .. 3}, 4 x 256 x 256 (1024 tiles, a few per persistent
                   workgroup): wherever a workgroup meets a larger r after a smaller one its dW exponent has to move
  tiny_all         every sample 1e-6 x randn: grad_w keeps the same relative bar (it sums over samples: no per-sample metric)
Reference semantics: GroupNorm(1, C) / Conv2d / SELU of ResNetBlock and Block2D3D (model/multi_frame_networks.py:338-345, 514-542)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SELU_L = 1.0507009873554804934193349852946
SELU_A = 1.6732632423543772848170429916717
EPS = 1e-5


def _lib():
    from depthinspace_amd import ops
    if ops.lib.fn('dis_get_conv_split')() != 1:
        pytest.skip('two-term fp16 kernels only')
    return ops


def _chw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _hwc(t):
    return t.permute(0, 2, 3, 1)


def _selu_grad(y):
    y = y.double().cpu()
    return torch.where(y > 0, torch.full_like(y, SELU_L), y + SELU_L * SELU_A)


def _dgrad64(g, wt):
    """input gradient of a 3 x 3 pad-1 conv with weight wt (cout, cin, 3, 3), NHWC in and out, double on the host"""
    gn = _chw(g)
    return _hwc(torch.nn.grad.conv2d_input((gn.shape[0], wt.shape[1], gn.shape[2], gn.shape[3]), wt.double().cpu(), gn, padding=1))


def _wgrad64(x, g, k=3, stride=1):
    xn, gn = _chw(x), _chw(g)
    gw = torch.nn.grad.conv2d_weight(xn, (gn.shape[1], xn.shape[1], k, k), gn, stride=stride, padding=1)
    return gw, gn.sum(dim=(0, 2, 3))


def _moments(st, n, m, eps):
    st = st.double().cpu().view(n, 2)
    mu = st[:, 0] / m
    var = (st[:, 1] / m - mu * mu).clamp_min(0.0)
    return mu, 1.0 / torch.sqrt(var + eps)


def _gn64(x, st, gam, bet, eps):
    """GroupNorm(1, C) from the given per-sample moments (NHWC), double"""
    n = x.shape[0]
    mu, r = _moments(st, n, x[0].numel(), eps)
    return (x.double().cpu() - mu.view(n, 1, 1, 1)) * r.view(n, 1, 1, 1) * gam.double().cpu() + bet.double().cpu()


def _gn_bwd64(g, q, st, gam, eps, in_act):
    """GroupNorm(1, C) backward from the per-sample moments of its input q and the per-(sample, channel) sums A = sum g,
    B = sum g q (what dis_gn_bwd_coef consumes): gpre (times SELU'(q) when q is also a SELU output), grad_gamma, grad_beta"""
    n = g.shape[0]
    m = g[0].numel()
    g64, q64, ga = g.double().cpu(), q.double().cpu(), gam.double().cpu()
    mu, r = _moments(st, n, m, eps)
    A, B = g64.sum(dim=(1, 2)), (g64 * q64).sum(dim=(1, 2))          # (n, c)
    gxa = (B - mu[:, None] * A) * r[:, None]                          # sum g xhat per (sample, channel)
    m1 = (ga * A).sum(1) / m                                          # mean of dL/dxhat
    m2 = (ga * gxa).sum(1) / m                                        # mean of dL/dxhat * xhat
    v = lambda t: t.view(n, 1, 1, 1)
    xh = (q64 - v(mu)) * v(r)
    gpre = v(r) * (g64 * ga - v(m1) - xh * v(m2))
    if in_act:
        gpre = gpre * _selu_grad(q64)
    return gpre, gxa.sum(0), A.sum(0)


def _ab64(g, abx, slots=None):
    """the channel sums of the conv epilogues, (n, 2, c): sum g, sum g * gn_x"""
    g64 = g.double().cpu()
    return torch.stack([g64.sum(dim=(1, 2)), (g64 * abx.double().cpu()).sum(dim=(1, 2))], 1)


def _err(a, ref, sel=None, norm=None):
    d, r = (a.double().cpu() - ref).abs(), ref.abs()
    if sel is not None:
        d, r = d[sel], r[sel]
    return float(d.max() / ((r.max() if norm is None else norm) + 1e-300))


def _judge(tag, a2, a3, ref, regions=(), per_sample=True):
    """a2 (f16x2) against a3 (bf16x3) on ref: globally, per sample, per region; 'rel' regions against their own largest entry,
    'abs' regions (tiny entries of tiles whose halo reaches O(1) values) printed locally and judged on their absolute error, of the
    largest entry overall: below 4 x the bf16x3 kernel's + 1e-9 (against the operand reference the bf16x3 term is ~1e-10: 1e-9 is
    the bar of test_conv_f16x2_dynamic_range; against fp64 both carry the same fp32 rounding of the formed operand)"""
    metrics = [('all', None, 'rel')]
    if per_sample and ref.dim() >= 2:
        for s in range(ref.shape[0]):
            sel = torch.zeros(ref.shape, dtype=torch.bool)
            sel[s] = True
            metrics.append(('sample %d' % s, sel, 'rel'))
    metrics += list(regions)
    out = []
    for name, sel, kind in metrics:
        e3, e2 = _err(a3, ref, sel), _err(a2, ref, sel)
        if kind == 'abs':
            ab3, ab2 = _err(a3, ref, sel, norm=float(ref.abs().max())), _err(a2, ref, sel, norm=float(ref.abs().max()))
            print(f'  {tag} [{name}] local relative: bf16x3 {e3:.2e}  f16x2 {e2:.2e}; absolute, of the largest entry: bf16x3 {ab3:.2e}  '
                  f'f16x2 {ab2:.2e}')
            out.append((tag, name, ab2 < 4 * ab3 + 1e-9, ab3, ab2))
            continue
        print(f'  {tag} [{name}]: bf16x3 {e3:.2e}  f16x2 {e2:.2e}')
        out.append((tag, name, e2 < 4 * e3 + 2e-7, e3, e2))
    bad = [o for o in out if not o[2]]
    assert not bad, bad


def _sel(shape, idx):
    s = torch.zeros(shape, dtype=torch.bool)
    s[idx] = True
    return s


def _regions(case, shape, outlier=None):
    n, h, w = shape[:3]
    if case == 'tiny_tiles':
        return [('all-tiny tile', _sel((n, h, w, shape[3]), (slice(None), slice(0, 15), slice(0, 15))), 'rel'),
                ('tiny, O(1) halo', _sel((n, h, w, shape[3]), (slice(None), slice(16, 31), slice(0, 31))) |
                 _sel((n, h, w, shape[3]), (slice(None), slice(0, 31), slice(16, 31))), 'abs')]
    if case == 'cancelling_gpre':
        return [('tiles away from the patches', _sel((n, h, w, shape[3]), (slice(None), slice(None), slice(32, None))), 'rel')]
    if case == 'outlier_pixel' and outlier is not None:
        s, y, x = outlier
        keep = torch.ones((n, h, w, shape[3]), dtype=torch.bool)
        keep[s, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
        return [('outputs that do not see the outlier', keep, 'rel')]
    return []


# ---------------------------------------------------------------- inputs of the GroupNorm-backward operand
def _patches(n, h, w, c, gen):
    """a few O(1) patches in the left 16 columns (the tiles from column 32 on never see them, halo included)"""
    p = torch.zeros(n, h, w, c)
    for s in range(n):
        for k in range(3):
            y0 = int(torch.randint(0, h - 4, (1,), generator=gen))
            x0 = 2 + 4 * k
            p[s, y0:y0 + 4, x0:x0 + 4] = torch.randn(4, 4, c, generator=gen)
    return p


def _gnb_inputs(case, n, h, w, c, in_act, gen):
    """q (GroupNorm input, a SELU output when in_act), g (gradient wrt the GroupNorm output), gamma, the moments of q, the sums ab0;
    the outlier of g (sample, y, x) for the region metric"""
    spread = 30.0 if case == 'cancelling_gpre' else 1.0   # (var >> eps: the xhat direction cancels too)
    q = torch.randn(n, h, w, c, generator=gen) * spread
    if in_act:
        q = F.selu(q)
    g = torch.randn(n, h, w, c, generator=gen)
    gamma = torch.rand(c, generator=gen) + 0.5
    st = torch.stack([q.double().sum(dim=(1, 2, 3)), (q.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
    outlier = None
    if case == 'outlier_pixel':
        g[1 % n, 7, 40, 3] = 1e4
        outlier = (1 % n, 7, 40)
    elif case == 'tiny_sample':
        g[1] *= 1e-6
    elif case == 'tiny_tiles':
        # dL/dxhat = alpha + beta xhat + z (z ~ randn) outside the 32 x 32 corner and a + b xhat + e (e ~ 1e-6 randn) inside it, with
        # (a, b) solved per sample so that they ARE the two means of the GroupNorm backward: gpre = rstd e there (1e-6), O(1) beside
        # it, while g stays O(1) in the corner too (a scale taken from g loses ~20 bits in the all-tiny tile)
        mu, r = _moments(st, n, h * w * c, EPS)
        vw = lambda t: t.view(n, 1, 1, 1)
        xh = (q.double() - vw(mu)) * vw(r)
        sgn = lambda: (torch.randint(0, 2, (n, 1, 1, 1), generator=gen) * 2 - 1).double()
        gxh = sgn() * (0.5 + torch.rand(n, 1, 1, 1, generator=gen).double()) + \
            sgn() * (0.5 + torch.rand(n, 1, 1, 1, generator=gen).double()) * xh + g.double()
        cor = (slice(None), slice(0, 32), slice(0, 32))
        e = torch.randn(n, 32, 32, c, generator=gen).double() * 1e-6
        m, mc = h * w * c, 32 * 32 * c
        outside = torch.ones(n, h, w, c, dtype=torch.bool)
        outside[cor] = False
        s1, s2 = (gxh * outside).sum(dim=(1, 2, 3)), (gxh * xh * outside).sum(dim=(1, 2, 3))
        xc = xh[cor]
        x1, x2 = xc.sum(dim=(1, 2, 3)), (xc * xc).sum(dim=(1, 2, 3))
        s1, s2 = s1 + e.sum(dim=(1, 2, 3)), s2 + (e * xc).sum(dim=(1, 2, 3))
        det = (m - mc) * (m - x2) - x1 * x1      # a (m - mc) - b x1 = s1,  -a x1 + b (m - x2) = s2
        a_, b_ = (s1 * (m - x2) + x1 * s2) / det, ((m - mc) * s2 + x1 * s1) / det
        gxh[cor] = vw(a_) + vw(b_) * xc + e
        g = (gxh / gamma.double()).float()
    elif case == 'cancelling_gpre':
        mu, r = _moments(st, n, h * w * c, EPS)
        xh = (q.double() - mu.view(n, 1, 1, 1)) * r.view(n, 1, 1, 1)
        sgn = lambda: (torch.randint(0, 2, (n, 1, 1, 1), generator=gen) * 2 - 1).double()
        al = sgn() * (0.5 + torch.rand(n, 1, 1, 1, generator=gen).double()) * 4e3
        be = sgn() * (0.5 + torch.rand(n, 1, 1, 1, generator=gen).double()) * 4e3
        g = ((al + be * xh) / gamma.double() + _patches(n, h, w, c, gen).double()).float()
    ab0 = torch.zeros(n, 2, c, dtype=torch.float64)
    ab0[:, 0] = g.double().sum(dim=(1, 2))
    ab0[:, 1] = (g.double() * q.double()).sum(dim=(1, 2))
    return q, g, gamma, st, ab0, outlier


def _coef(L, st, gamma, ab0, n, hw, c):
    slots = L.fn('dis_conv2d_gnsums_slots')()
    ab = torch.zeros(n, slots, 2, c, dtype=torch.float64, device='cuda')
    ab[:, 0] = ab0.cuda()
    coef = torch.empty(n * (c + 2) + 4 * n * c + 2, dtype=torch.float32, device='cuda')
    gg, gb = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    L.call('dis_gn_bwd_coef', st.cuda(), gamma.cuda(), ab, slots, coef, gg, gb, torch.zeros(2, dtype=torch.int32, device='cuda'), n, hw,
           c, EPS)
    return coef, gg, gb


def _print_cancel(g, gpre64, gpre32):
    away = (slice(None), slice(None), slice(32, None))
    g_ = float(g[away].abs().max())
    r64, r32 = float(gpre64[away].abs().max()) / g_, float(gpre32.double().cpu()[away].abs().max()) / g_
    print(f'  cancellation away from the patches: max|gpre| / max|g| = {r64:.2e} (fp64), {r32:.2e} (formed in fp32)')
    assert r64 < 1e-7 and r32 < 1e-7, (r64, r32)   # (1e-9 .. 1e-8 with these seeds)


def _check_gn_coef(gg, gb, gg64, gb64):
    for name, a, ref in (('grad_gamma', gg, gg64), ('grad_beta', gb, gb64)):
        e = _err(a, ref)
        print(f'  {name} of dis_gn_bwd_coef: {e:.2e} of the largest entry')
        assert e < 1e-6, (name, e)


# ---------------------------------------------------------------- dis_conv2d_dgrad_f16x2_gnb
@pytest.mark.parametrize('case', ['randn', 'outlier_pixel', 'tiny_sample', 'tiny_tiles', 'cancelling_gpre'])
@pytest.mark.parametrize('form,in_act', [('plain', 0), ('plain', 1), ('accum', 0), ('accum', 1), ('sums', 0), ('sums', 1),
                                         ('accum_sums_act', 1)])
@pytest.mark.parametrize('c', [16, 32])
def test_dgrad_gnb_against_fp64(c, form, in_act, case):
    """gpre and gx of the input-gradient launch with the GroupNorm backward formed on load, against fp64 and beside bf16x3 (the
    same gpre, materialised by dis_gn_bwd_apply_coef, through the three-term kernel); gpre, gx and the channel sums bit-identical
    to the two-launch form on the same adversarial data (the same scale decisions, not only the same arithmetic)"""
    from tests.conftest import conv_split
    ops = _lib()
    L = ops.lib
    n, h, w = 3, 64, 64
    gen = torch.Generator().manual_seed(11 * c + 3 * in_act + len(form) + 100 * len(case))
    q, g, gamma, st, ab0, outlier = _gnb_inputs(case, n, h, w, c, in_act, gen)
    wt = torch.randn(c, c, 3, 3, generator=gen) * 0.05
    accum, sums = form.startswith('accum'), 'sums' in form
    act_y = F.selu(torch.randn(n, h, w, c, generator=gen)) if form == 'accum_sums_act' else None
    gn_x = torch.randn(n, h, w, c, generator=gen) if sums else None
    base = torch.randn(n, h, w, c, generator=gen) * (0.0 if case == 'cancelling_gpre' else 1.0)
    if case == 'tiny_sample':
        base[1] *= 1e-6
    elif case == 'tiny_tiles':
        base[:, :32, :32] *= 1e-6
    qd, gd, wd = q.cuda(), g.cuda(), wt.cuda().contiguous()
    coef, gg, gb = _coef(L, st, gamma, ab0, n, h * w, c)
    slots = L.fn('dis_conv2d_gnsums_slots')()
    # ---- the fused launch
    gx = base.cuda()
    gpre = torch.full_like(gd, float('nan'))
    ab = torch.zeros(n * slots * 2 * c, dtype=torch.float64, device='cuda') if sums else None
    ok = L.call_try('dis_conv2d_dgrad_f16x2_gnb', gd, qd, coef, in_act, gpre, wd, c, c, wd.stride(0), gx, 1 if accum else 0,
                    gn_x.cuda() if sums else None, act_y.cuda() if act_y is not None else None, ab, n, h, w, c)
    assert ok, 'no instance for a production form'
    # ---- the two launches it replaces (two-term kernels), and the bf16x3 yardstick on the same materialised gpre

    def unfused():
        gpre_u = torch.empty_like(gd)
        L.call('dis_gn_bwd_apply_coef', gd, qd, coef, gpre_u, n, h * w, c, in_act)
        gx_u = base.cuda()
        ab_u = torch.zeros(n * slots * 2 * c, dtype=torch.float64, device='cuda') if sums else None
        if not sums:
            L.call('dis_conv2d_fwd_bf16x3_oihw', gpre_u, wd, 1, c, c, wd.stride(0), None, gx_u, None, n, h, w, c, c, 3, 1, 1,
                   ops.CONV_ACCUM if accum else 0)
        elif form == 'sums':
            L.call('dis_conv2d_dgrad_bf16x3_gnsums', gpre_u, wd, c, c, wd.stride(0), gx_u, gn_x.cuda(), ab_u, n, h, w, c, c, 1)
        else:
            L.call('dis_conv2d_dgrad_bf16x3_gnsums_res', gpre_u, wd, c, c, wd.stride(0), gx_u, act_y.cuda(), gn_x.cuda(), ab_u, n, h, w,
                   c, c, 1)
        return gpre_u, gx_u, ab_u
    gpre_u, gx_u, ab_u = unfused()
    with conv_split('bf16x3'):
        gpre3 = torch.empty_like(gd)
        L.call('dis_gn_bwd_apply_coef', gd, qd, coef, gpre3, n, h * w, c, in_act)
        gx3 = base.cuda()
        L.call('dis_conv2d_fwd_bf16x3_oihw', gpre3, wd, 1, c, c, wd.stride(0), None, gx3, None, n, h, w, c, c, 3, 1, 1,
               ops.CONV_ACCUM if accum else 0)
    torch.cuda.synchronize()
    assert torch.equal(gpre, gpre_u), float((gpre - gpre_u).abs().max())
    assert torch.equal(gx, gx_u), float((gx - gx_u).abs().max())
    if sums:
        assert torch.equal(ab, ab_u)
    assert torch.equal(gpre3, gpre)
    # ---- fp64
    gpre64, gg64, gb64 = _gn_bwd64(g, q, st, gamma, EPS, in_act)
    post = (lambda t: t) if act_y is None else (lambda t: t * _selu_grad(act_y))
    gx3 = gx3.double().cpu()
    if act_y is not None:
        gx3 = (gx3 * _selu_grad(act_y)).float().double()
    print(f'{case} c={c} {form} in_act={in_act}')
    if case == 'cancelling_gpre':
        _print_cancel(g, gpre64, gpre)
    _check_gn_coef(gg, gb, gg64, gb64)
    regions = _regions(case, (n, h, w, c), outlier)
    _judge('gpre vs fp64', gpre, gpre3, gpre64, regions=regions if case != 'cancelling_gpre' else ())
    for rname, op in (('fp64', gpre64), ('operand', gpre.double().cpu())):
        ref = post(_dgrad64(op, wt) + (base.double() if accum else 0.0))
        _judge('gx vs ' + rname, gx, gx3, ref, regions)
        if sums:
            a64 = _ab64(ref, gn_x)
            got = ab.view(n, slots, 2, c).sum(dim=1)
            _judge('channel sums vs ' + rname, got, _ab64(gx3, gn_x), a64)


# ---------------------------------------------------------------- GroupNorm on load, forward
def _exact_gn(case, n, h, w, c, gen):
    """(x, stats, gamma, beta, eps) whose fp32 normalisation is exact; None for the cases that use measured moments"""
    m = h * w * c
    if case == 'tiny_gn_output':
        # moments given as mean 0, variance 1 - 2^-16, eps 2^-16 (rstd 1), gamma 1, beta_c = -x0_c: the 32 x 32 corner holds
        # x0_c + 2^-20 k (k >= 1), so its normalised values are 2^-20 k exactly while the raw input is O(1).  (Values formed by
        # cancelling O(1) terms carry the fp32 grid of those terms - here 2 bits - and every fp16 scale in range holds them exactly:
        # this case checks the tile next to O(1) tiles and the statistics, it cannot see a scale sized from raw x.)
        x = torch.round(torch.randn(n, h, w, c, generator=gen) * 2 ** 12) * 2.0 ** -12
        x0 = torch.round(torch.randn(c, generator=gen) * 4) / 4
        k = torch.randint(1, 4, (n, 32, 32, c), generator=gen).float()
        x[:, :32, :32] = x0 + k * 2.0 ** -20
        st = torch.tensor([[0.0, m * (1.0 - 2.0 ** -16)]] * n, dtype=torch.float64).reshape(-1)
        return x, st, torch.ones(c), -x0, 2.0 ** -16
    return None


def _gn_fwd_inputs(case, n, h, w, c, gen):
    ex = _exact_gn(case, n, h, w, c, gen)
    if ex is not None:
        return ex
    if case == 'offset_gn_input':
        # x = 1000 + z with its measured moments, GroupNorm gain +-(0.5 .. 1) 2^-20 and shift 0.3 z 2^-20: the formed values
        # x * (rstd gamma) + (beta - rstd gamma mean) are ~3e-6 with ~14 significant bits (the fp32 grid of x * rstd gamma ~ 2^-10),
        # the raw ones 1e3 - a tile scale sized from raw x leaves them 4 (dW, 6 bits of headroom) to 10 (forward) bits
        x = 1000.0 + torch.randn(n, h, w, c, generator=gen)
        st = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
        gam = (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float() * (0.5 + 0.5 * torch.rand(c, generator=gen)) * 2.0 ** -20
        return x, st, gam, 0.3 * torch.randn(c, generator=gen) * 2.0 ** -20, EPS
    x = torch.randn(n, h, w, c, generator=gen) * 1.5 + 0.3
    if case == 'outlier_pixel':
        x[0, 20, 21, :] = 1e4
    elif case == 'tiny_sample':
        x[1] *= 1e-6
    st = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
    return x, st, 1 + 0.2 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen), EPS


def _gn_formed(L, x, st, gam, bet, eps):
    """GroupNorm(x) as the kernels form it on load, in fp32 (dis_gn_apply: the same moments, the same x * sc + sh)"""
    n, h, w, c = x.shape
    y = torch.empty(n, h, w, c, device='cuda')
    L.call('dis_gn_apply', x.cuda(), st.cuda(), gam.cuda(), bet.cuda(), None, y, n, h * w, c, 0, float(eps))
    return y.double().cpu()


def _fwd_regions(case, shape):
    n, h, w, c = shape
    if case == 'tiny_gn_output':
        return [('all-tiny tile', _sel(shape, (slice(None), slice(0, 15), slice(0, 15))), 'rel')]
    return []


@pytest.mark.parametrize('case', ['randn', 'outlier_pixel', 'tiny_sample', 'offset_gn_input', 'tiny_gn_output'])
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('c', [16, 32])
def test_conv_gn_in_forward_against_fp64(c, act, case):
    """ops.conv2d_gn_in's launch (dis_conv2d_fwd_bf16x3_gn: GroupNorm applied while the input is staged, tile scale of the formed
    values) and its output statistics against fp64, beside the three-term kernel on the same entry point"""
    from tests.conftest import conv_split
    ops = _lib()
    L = ops.lib
    n, h, w = 3, 64, 64
    gen = torch.Generator().manual_seed(5 * c + act + 100 * len(case))
    x, st, gam, bet, eps = _gn_fwd_inputs(case, n, h, w, c, gen)
    wt = torch.randn(c, c, 3, 3, generator=gen) / (3 * c ** 0.5)
    # (the bias at the scale of the conv's output where that output is small: an O(1) bias would hide the conv's own error)
    b = 0.1 * torch.randn(c, generator=gen) * {'tiny_gn_output': 1e-6, 'offset_gn_input': 2.0 ** -20}.get(case, 1.0)
    out = {}
    for tag in ('bf16x3', 'f16x2'):
        with conv_split(tag):
            y = torch.empty(n, h, w, c, device='cuda')
            ys = torch.zeros(2 * n, dtype=torch.float64, device='cuda')
            L.call('dis_conv2d_fwd_bf16x3_gn', x.cuda(), st.cuda(), gam.cuda(), bet.cuda(), eps, wt.cuda(), c, c, 0, b.cuda(), y, ys,
                   n, h, w, c, c, 3, 1, 1, act)
            out[tag] = (y, ys)
    xop = _gn_formed(L, x, st, gam, bet, eps)
    torch.cuda.synchronize()
    print(f'{case} c={c} act={act}')
    for rname, op in (('fp64', _gn64(x, st, gam, bet, eps)), ('operand', xop)):
        y64 = _hwc(F.conv2d(_chw(op), wt.double(), b.double(), padding=1))
        if act:
            y64 = F.selu(y64)
        _judge('y vs ' + rname, out['f16x2'][0], out['bf16x3'][0], y64, _fwd_regions(case, (n, h, w, c)))
        s64 = torch.stack([y64.sum(dim=(1, 2, 3)), (y64 ** 2).sum(dim=(1, 2, 3))], 1)
        _judge('output statistics vs ' + rname, out['f16x2'][1].view(n, 2), out['bf16x3'][1].view(n, 2), s64)


@pytest.mark.parametrize('case', ['randn', 'outlier_pixel', 'offset_gn_input', 'tiny_gn_output'])
def test_conv_gnres_forward_against_fp64(case):
    """dis_conv2d_fwd_f16x2_gnres: out = SELU(GroupNorm(x2) + res) formed on load (and stored), y = SELU(conv(out) + b) with its
    statistics - against fp64, beside dis_gn_apply + the three-term kernel"""
    from tests.conftest import conv_split
    ops = _lib()
    L = ops.lib
    n, h, w, c = 3, 64, 64, 32
    gen = torch.Generator().manual_seed(300 + len(case))
    x2, st, gam, bet, eps = _gn_fwd_inputs(case, n, h, w, c, gen)
    res = torch.randn(n, h, w, c, generator=gen)
    if case == 'tiny_gn_output':
        res[:, :32, :32] = 0.0
    elif case == 'offset_gn_input':
        res *= 2.0 ** -20
    wt = torch.randn(c, c, 3, 3, generator=gen) / (3 * c ** 0.5)
    # (the bias at the scale of the conv's output where that output is small: an O(1) bias would hide the conv's own error)
    b = 0.1 * torch.randn(c, generator=gen) * {'tiny_gn_output': 1e-6, 'offset_gn_input': 2.0 ** -20}.get(case, 1.0)
    ys = torch.zeros(2 * n, dtype=torch.float64, device='cuda')
    y, o = torch.empty(n, h, w, c, device='cuda'), torch.full((n, h, w, c), float('nan'), device='cuda')
    ok = L.call_try('dis_conv2d_fwd_f16x2_gnres', x2.cuda(), st.cuda(), gam.cuda(), bet.cuda(), eps, res.cuda(), o, wt.cuda(), c, c, 0,
                    b.cuda(), y, ys, n, h, w, c, c, ops.ACT_SELU)
    assert ok, 'no instance for a production form'
    with conv_split('bf16x3'):
        o3, y3 = torch.empty(n, h, w, c, device='cuda'), torch.empty(n, h, w, c, device='cuda')
        ys3 = torch.zeros(2 * n, dtype=torch.float64, device='cuda')
        L.call('dis_gn_apply', x2.cuda(), st.cuda(), gam.cuda(), bet.cuda(), res.cuda(), o3, n, h * w, c, ops.ACT_SELU, eps)
        L.call('dis_conv2d_fwd_bf16x3_oihw', o3, wt.cuda(), 0, c, c, 0, b.cuda(), y3, ys3, n, h, w, c, c, 3, 1, 1, ops.ACT_SELU)
    torch.cuda.synchronize()
    assert torch.equal(o, o3), float((o - o3).abs().max())
    o64 = F.selu(_gn64(x2, st, gam, bet, eps) + res.double())
    print(case)
    regions = _fwd_regions(case, (n, h, w, c))
    _judge('block output vs fp64', o, o3, o64, regions)
    for rname, op in (('fp64', o64), ('operand', o.double().cpu())):
        y64 = F.selu(_hwc(F.conv2d(_chw(op), wt.double(), b.double(), padding=1)))
        _judge('y vs ' + rname, y, y3, y64, regions)
        s64 = torch.stack([y64.sum(dim=(1, 2, 3)), (y64 ** 2).sum(dim=(1, 2, 3))], 1)
        _judge('statistics vs ' + rname, ys.view(n, 2), ys3.view(n, 2), s64)


# ---------------------------------------------------------------- dis_conv2d_wgrad_k4s2_f16x2_gnb
@pytest.mark.parametrize('case', ['randn', 'outlier_pixel', 'tiny_sample', 'cancelling_gpre'])
@pytest.mark.parametrize('in_act', [0, 1])
def test_wgrad_k4s2_gnb_against_fp64(in_act, case):
    """the 4 x 4 stride-2 weight gradient with gpre formed on load: grad_w, grad_b against fp64 beside dis_gn_bwd_apply_coef + the
    exact-fp32 kernel the three-term mode keeps for this shape; fixed bar 1e-6 of the largest entry against the operand reference"""
    from tests.conftest import conv_split
    ops = _lib()
    L = ops.lib
    n, h, w, c = 3, 128, 128, 32
    ho, wo = h // 2, w // 2
    gen = torch.Generator().manual_seed(70 + in_act + len(case))
    q, g, gamma, st, ab0, _ = _gnb_inputs(case, n, ho, wo, c, in_act, gen)
    x = torch.randn(n, h, w, c, generator=gen)
    if case == 'outlier_pixel':
        x[0, 20, 21, :] = 1e4
    elif case == 'tiny_sample':
        x[1] *= 1e-6
    coef, gg, gb_c = _coef(L, st, gamma, ab0, n, ho * wo, c)
    wsz = L.fn('dis_conv2d_wgrad_workspace')(c, c, 4, 2)
    gpre = torch.full((n, ho, wo, c), float('nan'), device='cuda')
    gw, gb = torch.empty(c, c, 4, 4, device='cuda'), torch.empty(c, device='cuda')
    L.call('dis_conv2d_wgrad_k4s2_f16x2_gnb', x.cuda(), g.cuda(), q.cuda(), coef, in_act, gpre, gw, gb, torch.empty(wsz, device='cuda'),
           n, h, w)
    with conv_split('bf16x3'):
        gpre3 = torch.empty_like(gpre)
        L.call('dis_gn_bwd_apply_coef', g.cuda(), q.cuda(), coef, gpre3, n, ho * wo, c, in_act)
        gw3, gb3 = torch.empty(c, c, 4, 4, device='cuda'), torch.empty(c, device='cuda')
        L.call('dis_conv2d_wgrad', x.cuda(), gpre3, gw3, gb3, torch.empty(wsz, device='cuda'), n, h, w, c, c, c, 4, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(gpre, gpre3)
    gpre64, gg64, gb64_c = _gn_bwd64(g, q, st, gamma, EPS, in_act)
    print(f'{case} in_act={in_act}')
    if case == 'cancelling_gpre':
        _print_cancel(g, gpre64, gpre)
    _check_gn_coef(gg, gb_c, gg64, gb64_c)
    for rname, op in (('fp64', gpre64), ('operand', gpre.double().cpu())):
        gw64, gb64 = _wgrad64(x, op, 4, 2)
        _judge('grad_w vs ' + rname, gw, gw3, gw64, per_sample=False)
        _judge('grad_b vs ' + rname, gb, gb3, gb64, per_sample=False)
        if rname == 'operand':
            for name, a, ref in (('grad_w', gw, gw64), ('grad_b', gb, gb64)):
                assert _err(a, ref) < 1e-6, (name, _err(a, ref))


# ---------------------------------------------------------------- dis_conv2d_bwd_fused_f16x2
FORMS = {   # name: (coef, in_act, accum, sums, xgn, store, chain)
    'plain': (False, 0, False, False, False, False, False),
    'plain_act': (False, 1, False, False, False, False, False),
    'coef': (True, 0, False, False, False, False, False),
    'coef_act_sums_xgn': (True, 1, False, True, True, False, False),
    'coef_sums_xgn_store': (True, 0, False, True, True, True, False),
    'chain': (True, 1, True, True, False, False, True),
}
FB_CASES = [(f, k) for f in FORMS for k in ('randn', 'outlier_pixel', 'tiny_sample', 'tiny_all')] + \
           [(f, 'tiny_tiles') for f in FORMS] + \
           [(f, 'cancelling_gpre') for f in FORMS if FORMS[f][0]] + \
           [(f, 'offset_gn_input') for f in FORMS if FORMS[f][4]]


def _run_fused(L, ops, form, case, n, h, w, gen, print_ramp=None):
    c = 32
    coef_form, in_act, accum, sums, xgn, store, chain = FORMS[form]
    outlier = None
    # ---- the operand: g and the GroupNorm backward's q (coef forms), or gy (act': q is the SELU output)
    if coef_form:
        q, g, gamma, st, ab0, outlier = _gnb_inputs('randn' if case in ('tiny_all', 'exponent_ramp') else case, n, h, w, c, in_act, gen)
    else:
        q = F.selu(torch.randn(n, h, w, c, generator=gen)) if in_act else None
        g = torch.randn(n, h, w, c, generator=gen)
        if case == 'outlier_pixel':
            g[1, 7, 40, 3] = 1e4
            outlier = (1, 7, 40)
        elif case == 'tiny_sample':
            g[1] *= 1e-6
        elif case == 'tiny_tiles':
            g[:, :32, :32] *= 1e-6
    # ---- the conv input x (GroupNorm input in the xgn forms, SELU output in the chain form)
    xg = None
    if case == 'offset_gn_input':
        x, xst, xgam, xbet, xeps = _gn_fwd_inputs(case, n, h, w, c, gen)
        xg = (xst, xgam, xbet, xeps)
    else:
        x = torch.randn(n, h, w, c, generator=gen) * 2.0 + 0.3
        if chain:
            x = F.selu(x)
        if case == 'outlier_pixel':
            x[0, 20, 21, :] = 1e4 if not chain else 1e4 * SELU_L
        elif case == 'tiny_sample':
            x[1] *= 1e-6
        elif case == 'tiny_tiles':
            x[:, :32, :32] *= 1e-6
        if xgn:
            xst = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
            xg = (xst, torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.1, EPS)
    if case in ('tiny_all', 'exponent_ramp'):
        if case == 'tiny_all':
            sc = torch.full((n, h, w, 1), 1e-6)
        else:   # 2^(7 r) per 16 x 16 tile, on x and on g
            r = torch.randint(0, 4, (n, (h + 15) // 16, (w + 15) // 16), generator=gen)
            sc = (2.0 ** (7 * r)).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :h, :w, None].float()
            print_ramp(r)
        g = g * sc
        x = x * sc
        if coef_form:   # the sums of the scaled g
            ab0 = torch.stack([g.double().sum(dim=(1, 2)), (g.double() * q.double()).sum(dim=(1, 2))], 1)
        if xgn:
            xst = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
            xg = (xst,) + xg[1:]
    ab_x = act_y = None
    if sums and not chain:
        ab_x = x          # conv2d_gn_in: the GroupNorm input of the sums IS the conv's input
    elif chain:
        ab_x = torch.randn(n, h, w, c, generator=gen)
        act_y = x
    wt = torch.randn(c, c, 3, 3, generator=gen) * 0.05
    base = torch.randn(n, h, w, c, generator=gen) * (0.0 if case in ('cancelling_gpre', 'tiny_all') else 1.0)
    if case == 'tiny_sample':
        base[1] *= 1e-6
    elif case == 'tiny_tiles':
        base[:, :32, :32] *= 1e-6
    dv = lambda t: t.cuda() if t is not None else None
    gd, qd, xd, wd, abxd, actd = dv(g), dv(q), dv(x), dv(wt).contiguous(), dv(ab_x), dv(act_y)
    abxd = xd if ab_x is x else abxd     # (the launch recognises the shared operand by its address)
    actd = xd if act_y is x else actd
    slots = L.fn('dis_conv2d_gnsums_slots')()
    coef = gg = gb_c = None
    if coef_form:
        coef, gg, gb_c = _coef(L, st, gamma, ab0, n, h * w, c)
    elif in_act:   # identity coefficients: dis_gn_bwd_apply_coef forms g * SELU'(q) with the kernels' own arithmetic
        coef = torch.zeros(n * (c + 2) + 4 * n * c + 2, device='cuda')
        coef[:n * (c + 2)].view(n, c + 2)[:, :c] = 1.0
    xgd = tuple(dv(t) if torch.is_tensor(t) else t for t in xg) if xgn else (None, None, None, EPS)
    # ---- the fused launch
    gx = base.cuda()
    gpre = torch.full_like(gd, float('nan')) if store else None
    ab = torch.zeros(n * slots * 2 * c, dtype=torch.float64, device='cuda') if sums else None
    gw, gb = torch.full((c, c, 3, 3), float('nan'), device='cuda'), torch.full((c,), float('nan'), device='cuda')
    ws = torch.empty(L.fn('dis_conv2d_bwd_fused_workspace')(c), dtype=torch.float32, device='cuda')
    ok = L.call_try('dis_conv2d_bwd_fused_f16x2', gd, qd, coef if coef_form else None, in_act, gpre, wd, c, c, wd.stride(0), gx,
                    1 if accum else 0, abxd, actd, ab, xd, xgd[0], xgd[1], xgd[2], float(xgd[3]), gw, gb, ws, n, h, w, c, 0)
    assert ok, 'no instance for a production form'
    # ---- the unfused two-term input gradient (bit-equality: the same scale decisions on this data)
    gx_u = base.cuda()
    if coef_form:
        gpre_u = torch.empty_like(gd)
        ab_u = torch.zeros(n * slots * 2 * c, dtype=torch.float64, device='cuda') if sums else None
        assert L.call_try('dis_conv2d_dgrad_f16x2_gnb', gd, qd, coef, in_act, gpre_u, wd, c, c, wd.stride(0), gx_u, 1 if accum else 0,
                          abxd, actd, ab_u, n, h, w, c)
    elif in_act:
        L.call('dis_conv2d_dgrad_bf16x3_act', gd, qd, in_act, wd, c, c, wd.stride(0), gx_u, n, h, w, c, c, 1, 0)
    else:
        L.call('dis_conv2d_fwd_bf16x3_oihw', gd, wd, 1, c, c, wd.stride(0), None, gx_u, None, n, h, w, c, c, 3, 1, 1, 0)
    # ---- bf16x3 yardstick: the materialised operand through the three-term kernels
    from tests.conftest import conv_split
    with conv_split('bf16x3'):
        if coef_form or in_act:
            gpre3 = torch.empty_like(gd)
            L.call('dis_gn_bwd_apply_coef', gd, qd, coef, gpre3, n, h * w, c, in_act)
        else:
            gpre3 = gd
        gx3 = base.cuda()
        L.call('dis_conv2d_fwd_bf16x3_oihw', gpre3, wd, 1, c, c, wd.stride(0), None, gx3, None, n, h, w, c, c, 3, 1, 1,
               ops.CONV_ACCUM if accum else 0)
        gw3, gb3 = torch.empty(c, c, 3, 3, device='cuda'), torch.empty(c, device='cuda')
        ws3 = torch.empty(L.fn('dis_conv2d_wgrad_workspace')(c, c, 3, 1), dtype=torch.float32, device='cuda')
        if xgn:
            L.call('dis_conv2d_wgrad_bf16x3_gn', xd, xgd[0], xgd[1], xgd[2], float(xgd[3]), gpre3, gw3, gb3, ws3, n, h, w, c, c, c, 3, 1, 1)
        else:
            L.call('dis_conv2d_wgrad_bf16x3', xd, gpre3, gw3, gb3, ws3, n, h, w, c, c, c, 3, 1, 1)
    torch.cuda.synchronize()
    assert torch.equal(gx, gx_u), float((gx - gx_u).abs().max())
    if coef_form:
        assert torch.equal(gpre3, gpre_u)
        if sums:
            got, ref = ab.view(n, slots, 2, c).sum(dim=1), ab_u.view(n, slots, 2, c).sum(dim=1)
            assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    if store:
        assert torch.equal(gpre, gpre3)
    gx3 = gx3.double().cpu()
    if chain:
        gx3 = (gx3 * _selu_grad(act_y)).float().double()
    # ---- fp64
    if coef_form:
        gpre64, gg64, gb64_c = _gn_bwd64(g, q, st, gamma, EPS, in_act)
        if case == 'cancelling_gpre':
            _print_cancel(g, gpre64, gpre3)
        _check_gn_coef(gg, gb_c, gg64, gb64_c)
    else:
        gpre64 = g.double() * (_selu_grad(q) if in_act else 1.0)
    xs = {'fp64': _gn64(x, *xg) if xgn else x.double(), 'operand': _gn_formed(L, x, *xg) if xgn else x.double()}
    post = (lambda t: t * _selu_grad(act_y)) if chain else (lambda t: t)
    regions = _regions(case, (n, h, w, c), outlier)
    if store:
        _judge('stored gpre vs fp64', gpre, gpre3, gpre64, () if case == 'cancelling_gpre' else regions)
    res = {}
    for rname, op in (('fp64', gpre64), ('operand', gpre3.double().cpu())):
        gx64 = post(_dgrad64(op, wt) + (base.double() if accum else 0.0))
        _judge('gx vs ' + rname, gx, gx3, gx64, regions)
        if sums:
            _judge('channel sums vs ' + rname, ab.view(n, slots, 2, c).sum(dim=1), _ab64(gx3, ab_x), _ab64(gx64, ab_x))
        gw64, gb64 = _wgrad64(xs[rname], op)
        e = [_err(gw, gw64), _err(gw3, gw64), _err(gb, gb64), _err(gb3, gb64)]
        print(f'  grad_w vs {rname}, of the largest entry: f16x2 fused {e[0]:.2e}, bf16x3 {e[1]:.2e}; grad_b {e[2]:.2e} / {e[3]:.2e}')
        assert e[0] < 4 * e[1] + 2e-7 and e[2] < 4 * e[3] + 2e-7, e
        res[rname] = e
    assert res['operand'][0] < 1e-6 and res['operand'][2] < 1e-6, res['operand']
    return res


@pytest.mark.parametrize('form,case', FB_CASES)
def test_bwd_fused_against_fp64(form, case):
    """dis_conv2d_bwd_fused_f16x2 in the forms the step uses: gx (and the stored gpre) against fp64 globally / per sample / per
    region, grad_w / grad_b within 1e-6 of the largest entry, the channel sums against fp64 - and gx still bit-identical to the
    unfused two-term launch on the same adversarial data"""
    ops = _lib()
    print(f'{form} {case}')
    _run_fused(ops.lib, ops, form, case, 3, 64, 64, torch.Generator().manual_seed(900 + 13 * len(form) + len(case)))


@pytest.mark.parametrize('form', ['plain', 'coef'])
def test_bwd_fused_dw_exponent_ramp(form):
    """exponent_ramp: x and gy scaled per 16 x 16 tile by 2^(7 r), r in {0 .. 3} drawn per tile (products spread over 2^42).  1024
    tiles over the persistent workgroups give each a few tiles; a workgroup that meets a larger r after a smaller one (a jump of
    2^14 .. 2^42, far past the FB_SMARGIN headroom) must flush its dW accumulators and restart with a new exponent, and many do -
    how many is not observable from outside the launch (a restart check that misses tiles up to 2^8 past the headroom fails this
    test).  grad_w / grad_b stay within 1e-6 of the largest entry and within 4 x the bf16x3 kernel's error."""
    ops = _lib()
    n, h, w = 4, 256, 256

    def show(r):
        cnt = [int((r == k).sum()) for k in range(4)]
        print(f'{form} exponent_ramp: {r.numel()} tiles, tile scales 2^0 .. 2^21 on x and on gy (products 2^0 .. 2^42); '
              f'tiles per r: {cnt}')
        assert min(cnt) > 0
    _run_fused(ops.lib, ops, form, 'exponent_ramp', n, h, w, torch.Generator().manual_seed(4242 + len(form)), show)
