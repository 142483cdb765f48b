"""CPU: the host side of the device-resident optimiser hyper-parameters - trainer.LRSchedule / step_decay against torch's own
LambdaLR, the command-line flags, FlatAdam's param_groups surface, and the argument checks of dis_adam_step_hyper (every refusal
below returns before anything is launched, so no GPU is needed: the library is reached as tests/test_abi.py reaches it)."""
import ctypes
import os

import pytest
import torch


def _lib():
    import __graft_entry__ as g
    from depthinspace_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    return lib


@pytest.mark.parametrize('name', ['step_decay', 'warmup_cosine'])
def test_lr_schedule_follows_lambda_lr(name):
    import math
    from depthinspace_amd.trainer import LRSchedule, step_decay
    lam = {'step_decay': step_decay(3, 0.5),
           'warmup_cosine': lambda e: min(1.0, (e + 1) / 4) * 0.5 * (1 + math.cos(math.pi * e / 12))}[name]
    mine = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=3e-4)
    ref = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=3e-4)
    s_mine = LRSchedule(mine, lam)
    s_ref = torch.optim.lr_scheduler.LambdaLR(ref, lam)
    for epoch in range(12):
        assert mine.param_groups[0]['lr'] == ref.param_groups[0]['lr'], epoch
        assert s_mine.get_last_lr() == s_ref.get_last_lr()
        assert s_mine.last_epoch == s_ref.last_epoch == epoch
        ref.step()
        s_mine.step()
        s_ref.step()
    if name == 'step_decay':
        assert mine.param_groups[0]['lr'] == 3e-4 * 0.5 ** 4
    # a restored schedule continues where the saved one was
    fresh = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=3e-4)
    s2 = LRSchedule(fresh, lam)
    s2.load_state_dict(s_mine.state_dict())
    assert s2.last_epoch == 12 and s2.get_last_lr() == s_mine.get_last_lr()
    s2.step()
    s_ref.step()
    assert fresh.param_groups[0]['lr'] == ref.param_groups[0]['lr']


def test_step_decay_arithmetic():
    from depthinspace_amd.trainer import step_decay
    f = step_decay(10, 0.5)
    assert [f(e) for e in (0, 9, 10, 19, 20, 35)] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.125]
    assert step_decay(1, 0.1)(3) == 0.1 ** 3
    with pytest.raises(ValueError):
        step_decay(0, 0.5)


def test_optimiser_flags_defaults_and_parsing():
    from depthinspace_amd.co.args import parse_args
    a = parse_args([])
    assert a.lr == 1e-4 and a.lr_step == 0 and a.lr_gamma == 0.5 and a.max_grad_norm is None and a.skip_nonfinite is False
    a = parse_args(['--lr', '3e-4', '--lr_step', '20', '--lr_gamma', '0.1', '--max_grad_norm', '2.5', '--skip_nonfinite', 'true'])
    assert a.lr == 3e-4 and a.lr_step == 20 and a.lr_gamma == 0.1 and a.max_grad_norm == 2.5 and a.skip_nonfinite is True
    assert a.architecture == 'single_frame' and a.train_batch_size == 8       # (the reference's flags keep their defaults)
    with pytest.raises(SystemExit):
        parse_args(['--max_grad_norm', 'none'])


def test_flat_adam_param_groups_surface():
    """host side only (CPU tensors; the step itself is HIP-only and refuses them)"""
    _lib()
    from depthinspace_amd.trainer import FlatAdam, LRSchedule
    opt = FlatAdam([torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))], lr=1e-3, world_size=1)
    assert isinstance(opt.param_groups, list) and len(opt.param_groups) == 1 and type(opt.param_groups[0]) is dict
    g = opt.param_groups[0]
    assert g['lr'] == 1e-3 and g['betas'] == (0.9, 0.999) and g['eps'] == 1e-8 and g['params'] == [0, 1]
    assert opt.mode == 0 and opt.partials is None
    for grp in opt.param_groups:
        grp['lr'] *= 0.5
    assert opt.lr == 5e-4
    opt.lr = 2e-4
    assert g['lr'] == 2e-4 and opt.state_dict()['param_groups'][0]['lr'] == 2e-4
    # plain Adam writes exactly the keys it wrote before the clip / skip options existed
    assert list(opt.state_dict()['param_groups'][0]) == ['lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach',
                                                         'capturable', 'differentiable', 'fused', 'params']
    with pytest.raises(TypeError):
        torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0)      # why LRSchedule exists
    s = LRSchedule(opt, lambda e: 0.1 ** e)
    s.step()
    assert opt.lr == 2e-4 * 0.1
    with pytest.raises(ValueError):
        opt.max_grad_norm = 1.0
    clip = FlatAdam([torch.nn.Parameter(torch.zeros(5))], max_grad_norm=2.0, skip_nonfinite=True, world_size=1)
    assert clip.mode == 3 and clip.partials.dtype == torch.float64 and clip.partials.numel() == 1
    sd = clip.state_dict()['param_groups'][0]
    assert sd['max_grad_norm'] == 2.0 and sd['skip_nonfinite'] is True
    clip.max_grad_norm = 0.5
    assert clip.param_groups[0]['max_grad_norm'] == 0.5
    with pytest.raises(ValueError):
        clip.max_grad_norm = None
    opt.load_state_dict({'state': {}, 'param_groups': [dict(sd, params=[0, 1], lr=7e-4)]})
    assert opt.mode == 3 and opt.max_grad_norm == 2.0 and opt.lr == 7e-4 and opt.partials.numel() == 1
    with pytest.raises(ValueError):
        opt.load_state_dict({'state': {}, 'param_groups': [dict(sd, params=[0, 1], amsgrad=True)]})


def test_adam_step_hyper_argument_checks():
    lib = _lib()
    f = lib.fn('dis_adam_step_hyper')
    buf = ctypes.create_string_buffer(256)      # never dereferenced: every call below is refused on the host
    P = ctypes.cast(buf, ctypes.c_void_p).value
    OK, BAD_SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -3

    def call(param=P, grad=P, m=P, v=P, count=8, hyper=P, state=P, stats=P, partials=P, mode=3):
        return f(param, grad, m, v, count, hyper, 0.9, 0.999, 1e-8, state, stats, partials, mode, 1.0, None)

    for k in ('param', 'grad', 'm', 'v', 'hyper', 'state'):
        assert call(**{k: None}) == NULL, k
        assert call(**{k: None}, mode=0) == NULL, k
    for mode in (1, 2, 3):
        assert call(stats=None, mode=mode) == NULL
        assert call(partials=None, mode=mode) == NULL
    assert call(count=0) == BAD_SHAPE and call(count=-4) == BAD_SHAPE and call(count=0, mode=0) == BAD_SHAPE
    assert call(count=6) == UNSUPPORTED and call(count=6, mode=0, stats=None, partials=None) == UNSUPPORTED
    for mode in (4, 8, 7, -1, 1 << 30):
        assert call(mode=mode) == UNSUPPORTED, mode
    assert OK == 0


def test_adam_step_hyper_workspace_query():
    lib = _lib()
    ws = lib.fn('dis_adam_step_hyper_workspace')
    assert ws.restype is ctypes.c_long
    for bad in (0, -4, 6, 1023):
        assert ws(bad) < 0, bad
    assert ws(4) == 1 and ws(332) == 1
    sizes = [ws(c) for c in (4, 1 << 10, 1 << 14, 1 << 18, 512 * 1024, 31_600_000, 1 << 31, 1 << 33)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert ws(1 << 33) == 2 * ws(1 << 32)       # one workgroup per fixed-size range: a function of the count alone
    # the chunk of one workgroup: where the count goes from 1 to 2 workgroups, k chunks need k
    chunk = 4
    while ws(chunk + 4) == 1:
        chunk += 4
    assert ws(3 * chunk) == 3 and ws(3 * chunk + 4) == 4
    assert ws(31_600_000) * 8 < (1 << 20)        # DIS-SF: the workspace stays small
