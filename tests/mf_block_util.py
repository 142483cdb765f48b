"""A seeded Block2D3D forward + backward on synthetic geometry, shared by the tests that switch one of its launches on and off."""
import torch


def block_run(tl, bs, h, w, seed=3):
    """one Block2D3D forward + backward on seeded inputs -> [output, grad wrt feat, every parameter gradient] (CPU)"""
    from depthinspace_amd import ops
    from depthinspace_amd.model.multi_frame_networks import Block2D3D
    C = 32
    torch.manual_seed(seed)
    blk = Block2D3D(C, tl).cuda()
    g = torch.Generator().manual_seed(seed + 10 * tl)
    xyz = torch.randn(tl, bs, h, w, tl, 3, generator=g) * 0.05
    xyz[..., 2] += 3.0
    xyz[..., 0] += (torch.arange(w).view(1, 1, 1, w, 1) - w / 2) * 0.01
    xyz[..., 1] += (torch.arange(h).view(1, 1, h, 1, 1) - h / 2) * 0.01
    mask = (torch.rand(tl, bs, h, w, tl, 1, generator=g) > 0.2).float()
    mask[:, :, :, :, 0] = 1
    geom = torch.cat([xyz, mask], -1).cuda().contiguous()
    hq, wq = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    geom_q = ops.mf_geometry_resize(geom, (hq, wq))
    flows = ((torch.rand(tl * tl, bs, h, w, 2, generator=g) - 0.5) * 8).cuda()
    flows_q = ((torch.rand(tl * tl, bs, hq, wq, 2, generator=g) - 0.5) * 4).cuda()
    idx, idx_q = ops.conv3d_select(geom, 2), ops.conv3d_select(geom_q, 1)
    csr, csr_q = ops.gather_csr(flows), ops.gather_csr(flows_q)
    feat = torch.randn(tl, bs, h, w, C, generator=g).cuda().requires_grad_(True)
    go = torch.randn(tl, bs, h, w, C, generator=g).cuda()
    out = blk(feat, geom, geom_q, flows, flows_q, idx, idx_q, csr, csr_q)
    out.backward(go)
    torch.cuda.synchronize()
    grads = [p.grad for _, p in sorted(blk.named_parameters())]
    assert all(gr is not None for gr in grads)
    return [out.detach().cpu(), feat.grad.cpu()] + [gr.cpu() for gr in grads]
