"""tests/head_ref.py against torch autograd in float64 (F.conv2d + sigmoid), on two ragged shapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_ref as H


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300))


@pytest.mark.parametrize('n,h,w,cin,offset', [(2, 5, 3, 16, 3.0), (1, 17, 23, 32, 0.5), (1, 1, 1, 16, 0.5)])
def test_head_ref_matches_torch_autograd(n, h, w, cin, offset):
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, h, w, cin, generator=g, dtype=torch.float64)
    wt = (torch.randn(1, cin, 3, 3, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    b = torch.randn(1, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)
    alpha = 128.0
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = alpha * torch.sigmoid(F.conv2d(xr, wt, b, padding=1) - offset)
    y.backward(gy)
    yn = H.forward(x.numpy(), wt.detach().numpy(), b.detach().numpy(), alpha, offset)
    assert yn.shape == (n, 1, h, w) and _rel(yn, y.detach().numpy()) < 1e-12
    gx, gw, gb = H.backward(x.numpy(), wt.detach().numpy(), yn, gy.numpy(), alpha)
    assert _rel(gx, xr.grad.permute(0, 2, 3, 1).numpy()) < 1e-12
    assert _rel(gw, wt.grad.numpy()) < 1e-12
    assert _rel(gb, b.grad.numpy()) < 1e-12
    # the sums over absolute values bound the signed ones
    ax, aw, ab = H.backward(x.numpy(), wt.detach().numpy(), yn, gy.numpy(), alpha, return_abs=True)[3:]
    assert np.all(ax >= np.abs(gx)) and np.all(aw >= np.abs(gw)) and np.all(ab >= np.abs(gb))


def test_head_ref_saturates_without_overflow():
    x = np.zeros((1, 3, 3, 16))
    x[0, 1, 1, 0] = 1.0
    w = np.zeros((1, 16, 3, 3))
    for z, want in ((1000.0, 128.0), (-1000.0, 0.0)):
        w[0, 0, 1, 1] = z
        with np.errstate(over='raise', invalid='raise', divide='raise'):
            y = H.forward(x, w, np.zeros(1), 128.0, 0.0)
        assert y[0, 0, 1, 1] == want and y[0, 0, 0, 0] == 64.0
