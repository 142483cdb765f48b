"""Same-process A/B of dis_conv2d_bwd_fused_f16x2_c16 against the two launches it replaces (input gradient + weight gradient, each
with its slab-reduce), per form, at a FuseNet layer's real shape (16 x h x w, cin -> cout) - HIP events, interleaved rounds.

    python scripts/diag/bwd_fused_c16_probe.py [reps] [h w] [cin cout]           (defaults: 10, 512 432, 16 16)
"""
import os
import sys
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from depthinspace_amd import ops

L = ops.lib
S = ops.ACT_SELU


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    h, w = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (512, 432)
    cin, cout = (int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (16, 16)
    n = 16
    g_ = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g_).cuda()
    q0 = rnd(n, h, w, cout)
    gq = rnd(n, h, w, cout)
    wt = (rnd(cout, cin, 3, 3) * 0.05).contiguous()
    x = rnd(n, h, w, cin)
    xs = F.selu(x)
    ab_other = rnd(n, h, w, cin)
    slots_old = L.fn('dis_conv2d_gnsums_slots')()
    slots_new = L.fn('dis_conv2d_bwd_fused_c16_slots')(cin, cout)
    wsz = L.fn('dis_conv2d_wgrad_workspace')(cin, cout, 3, 1)
    xst = torch.stack([x.double().sum(dim=(1, 2, 3)), (x.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
    xgam, xbet = (torch.rand(cin, generator=g_) + 0.5).cuda(), (torch.randn(cin, generator=g_) * 0.1).cuda()
    forms = {
        # name: (coef?, in_act, accum, ab_x, act_y, x, xgn)
        'plain': (False, 0, False, None, None, x, False),
        'plain_accum': (False, 0, True, None, None, x, False),
        'plain_act': (False, S, False, None, None, x, False),
    }
    if cin != cout:
        # final_conv / ref_conv's 16-channel source: gx = conv_T(gy selu'(y)) selu'(x) written, plus the channel sums (x fetched once)
        forms['act_sums_res'] = (False, S, False, ab_other, xs, xs, False)
    if cin == cout:
        gamma = (torch.rand(cout, generator=g_) + 0.5).cuda()
        forms.update({
            'coef_sums_xgn (ResNetBlock conv2)': (True, 0, False, x, None, x, True),
            'coef_act_sums_xgn': (True, S, False, x, None, x, True),
            'coef_act (block conv1, no residual sums)': (True, S, False, None, None, x, False),
            'coef_act_accum (first block conv1)': (True, S, True, None, None, x, False),
            'two_consumer': (True, S, True, ab_other, None, x, False),
            'chain (second block conv1)': (True, S, True, ab_other, xs, xs, False),
        })
    only = os.environ.get('PROBE_FORMS')
    rows = []
    for name, (cf, in_act, accum, ab_x, act_y, xx, xgn) in forms.items():
        if only and name.split()[0] not in only.split(','):
            continue
        q = F.selu(q0) if in_act else q0
        coef = None
        if cf:
            st = torch.stack([q.double().sum(dim=(1, 2, 3)), (q.double() ** 2).sum(dim=(1, 2, 3))], 1).reshape(-1).contiguous()
            ab0 = torch.zeros(n, slots_old, 2, cout, dtype=torch.float64, device='cuda')
            ab0[:, 0, 0] = gq.double().sum(dim=(1, 2))
            ab0[:, 0, 1] = (gq.double() * q.double()).sum(dim=(1, 2))
            coef = torch.empty(n * (cout + 2) + 4 * n * cout + 2, dtype=torch.float32, device='cuda')
            L.call('dis_gn_bwd_coef', st, gamma, ab0, slots_old, coef, torch.empty(cout, device='cuda'), torch.empty(cout, device='cuda'),
                   torch.zeros(2, dtype=torch.int32, device='cuda'), n, h * w, cout, 1e-5)
        gx = torch.zeros(n, h, w, cin, device='cuda')
        gpre = torch.empty_like(gq)
        ab_old = torch.zeros(n * slots_old * 2 * cin, dtype=torch.float64, device='cuda') if ab_x is not None else None
        ab_new = torch.zeros(n * slots_new * 2 * cin, dtype=torch.float64, device='cuda') if ab_x is not None else None
        gw, gb = torch.empty(cout, cin, 3, 3, device='cuda'), torch.empty(cout, device='cuda')
        ws = torch.empty(max(wsz, L.fn('dis_conv2d_bwd_fused_c16_workspace')(cin, cout)), dtype=torch.float32, device='cuda')
        acc = 1 if accum else 0

        def old():
            if cf:
                L.call('dis_conv2d_dgrad_f16x2_gnb', gq, q, coef, in_act, gpre, wt, cout, cin, wt.stride(0), gx, acc, ab_x, act_y, ab_old,
                       n, h, w, cin)
                gp = gpre
            elif in_act and ab_x is not None:
                L.call('dis_conv2d_dgrad_bf16x3_act_gnsums_res', gq, q, wt, cout, cin, wt.stride(0), gx, act_y, ab_x, ab_old, n, h, w,
                       cout, cin, 1)
                gp = None
            elif in_act:
                L.call('dis_conv2d_dgrad_bf16x3_act', gq, q, in_act, wt, cout, cin, wt.stride(0), gx, n, h, w, cout, cin, 1, acc)
                gp = None
            else:
                L.call('dis_conv2d_fwd_bf16x3_oihw', gq, wt, 1, cout, cin, wt.stride(0), None, gx, None, n, h, w, cout, cin, 3, 1, 1,
                       ops.CONV_ACCUM if accum else 0)
                gp = gq
            if xgn:
                L.call('dis_conv2d_wgrad_bf16x3_gn', xx, xst, xgam, xbet, 1e-5, gp, gw, gb, ws, n, h, w, cin, cin, cout, 3, 1, 1)
            elif gp is None:
                L.call('dis_conv2d_wgrad_bf16x3_act', xx, gq, q, in_act, gw, gb, ws, n, h, w, cin, cin, cout, 3, 1, 1)
            else:
                L.call('dis_conv2d_wgrad_bf16x3', xx, gp, gw, gb, ws, n, h, w, cin, cin, cout, 3, 1, 1)

        def new():
            return L.call_try('dis_conv2d_bwd_fused_f16x2_c16', gq, q if (cf or in_act) else None, coef, in_act, None, wt, cout, cin,
                              wt.stride(0), gx, acc, ab_x, act_y, ab_new, slots_new, xx, xst if xgn else None, xgam if xgn else None,
                              xbet if xgn else None, 1e-5, gw, gb, ws, n, h, w, 0)

        if not new():
            print(f'{name:48s} no instance')
            continue
        t = {'old': [], 'new': []}
        for r in range(reps + 2):
            for k, fn in (('old', old), ('new', new)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    t[k].append(e0.elapsed_time(e1) / 5 * 1e3)
        o, nw = sorted(t['old'])[len(t['old']) // 2], sorted(t['new'])[len(t['new']) // 2]
        rows.append((name, o, nw))
        print(f'{name:48s} two launches {o:7.1f} us   fused {nw:7.1f} us   ratio {nw / o:5.2f}', flush=True)
    return rows


if __name__ == '__main__':
    main()
