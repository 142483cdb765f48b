"""dis_adam_step_hyper and what trainer.FlatAdam builds on it: the learning rate, max_norm and the clip / skip decision live
on the device, so they work the same eagerly and under hipGraph replay, and the host changes them between replays without
re-capturing.  Shapes are the small ones of tests/test_net_ops_gpu.py::test_adam_graph_replay_matches_torch (and its bar of
5e-7 absolute on the parameters against torch.optim.Adam on the CPU), not the networks'."""
import argparse
import functools

import pytest
import torch

from depthinspace_amd.trainer import graph_capture   # (torch.cuda.graph with the cyclic collector held off: see its docstring)

pytestmark = pytest.mark.gpu

SHAPES = [(8, 4, 3, 3), (8,), (33,)]
N = 8 * 4 * 3 * 3 + 8 + 33      # 329 real elements, padded to 332 in the flat buffers
BAR = 5e-7


@functools.lru_cache(None)
def _counts():
    """4: one float4; 332: ragged against a 256-thread workgroup; and three norm workgroups with a ragged last one (77 float4),
    found from the workspace query: `chunk` is the largest count one workgroup covers"""
    from depthinspace_amd import lib
    ws = lib.fn('dis_adam_step_hyper_workspace')
    chunk = 4
    while ws(chunk + 4) == 1:
        chunk += 4
        assert chunk < (1 << 22)
    big = 2 * chunk + 4 * 77
    assert ws(4) == 1 and ws(332) == 1 and ws(2 * chunk) == 2 and ws(big) == 3
    return (4, 332, big)


def _make(lr=1e-3, seed=4, nsteps=6, **kw):
    """seeded parameters, per-step gradients (scaled by 10^-k), a torch.optim.Adam on CPU copies and a FlatAdam on the GPU"""
    from depthinspace_amd.trainer import FlatAdam
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s_, generator=g) for s_ in SHAPES]
    ref = [p.clone().requires_grad_(True) for p in ps]
    topt = torch.optim.Adam(ref, lr=lr)
    mine = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
    opt = FlatAdam(mine, lr=lr, **kw)
    grads = [[torch.randn(s_, generator=g) * 10 ** (-k) for s_ in SHAPES] for k in range(nsteps)]
    return ps, ref, topt, mine, opt, grads


def _flat(gr):
    return torch.cat([t.reshape(-1) for t in gr])


def _tensors(opt):
    return (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.state_dev, opt.stats_dev)


class _Stepper(object):
    """one optimiser step on a static gradient input `gin`: eager, or one captured step replayed.  The capture's eager warm-up
    step is undone (parameters, moments, step counter, statistics), so replay k is step k."""

    def __init__(self, opt):
        self.opt = opt
        self.gin = torch.zeros_like(opt.flat_g)
        self.graph = None

    def load(self, gr):
        flat = gr if torch.is_tensor(gr) else _flat(gr)
        self.gin[:self.opt.n].copy_(flat.cuda())

    def eager(self, gr):
        self.load(gr)
        self.opt.flat_g.copy_(self.gin)
        self.opt.step()

    def capture(self):
        opt = self.opt
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            snap = [t.clone() for t in _tensors(opt)]
            opt.flat_g.copy_(self.gin)
            opt.step()
            for t, c in zip(_tensors(opt), snap):
                t.copy_(c)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with graph_capture(self.graph):
            opt.flat_g.copy_(self.gin)
            opt.step(all_reduce=False)

    def replay(self, gr):
        self.load(gr)
        self.opt.sync_hyper()     # what GraphedStep.run() does in front of every replay
        self.graph.replay()


def _torch_step(ref, topt, gr, lr=None, max_norm=None):
    for r, t in zip(ref, gr):
        r.grad = t.clone()
    if lr is not None:
        topt.param_groups[0]['lr'] = lr
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
    topt.step()


def _maxdiff(mine, ref):
    return max(float((a.detach().cpu() - b.detach()).abs().max()) for a, b in zip(mine, ref))


# ------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize('which', [0, 1, 2])
def test_hyper_entry_point_is_bit_identical_to_adam_step_dev(which):
    """mode 0, and mode 1 with max_norm above every gradient norm (coefficient exactly 1), give the bits of dis_adam_step_dev"""
    from depthinspace_amd import lib, ops
    count = _counts()[which]
    g = torch.Generator().manual_seed(10 + which)
    p0 = torch.randn(count, generator=g).cuda()
    grads = [(torch.randn(count, generator=g) * 10 ** (-k)).cuda() for k in range(3)]
    hyper = torch.tensor([1e-3, 1e9, 0.0, 0.0], dtype=torch.float32).cuda()
    partials = torch.empty(lib.fn('dis_adam_step_hyper_workspace')(count), dtype=torch.float64, device='cuda')

    def run(mode):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        state = torch.zeros(4, dtype=torch.int32, device='cuda')
        stats = torch.zeros(4, dtype=torch.float64, device='cuda')
        for gr in grads:
            if mode is None:
                ops.adam_step_dev(p, gr, m, v, state, lr=1e-3)
            elif mode == 0:
                ops.adam_step_hyper(p, gr, m, v, state, hyper)   # stats / partials may be absent without a norm pass
            else:
                ops.adam_step_hyper(p, gr, m, v, state, hyper, stats, partials, mode)
        torch.cuda.synchronize()
        return p, m, v, state, stats

    old = run(None)
    for mode in (0, 1):
        new = run(mode)
        for a, b, name in zip(old[:4], new[:4], ('param', 'exp_avg', 'exp_avg_sq', 'state')):
            assert torch.equal(a, b), (count, mode, name)
        if mode == 1:
            assert float(new[4][1]) == 1.0 and float(new[4][2]) == 0.0 and float(new[4][3]) == 0.0
            ref = float(grads[-1].double().norm())
            assert abs(float(new[4][0]) - ref) <= 1e-10 * ref
    assert int(old[3][0]) == 3


# ------------------------------------------------------------------------------------------------ 2. lr after capture
def test_learning_rate_changed_after_capture_is_honoured():
    ps, ref, topt, mine, opt, grads = _make(lr=1e-3)
    st = _Stepper(opt)
    st.load(grads[0])
    st.capture()
    st.replay(grads[0])
    st.replay(grads[1])
    opt.lr = 5e-4
    st.replay(grads[2])
    opt.param_groups[0]['lr'] = 2.5e-4
    st.replay(grads[3])
    torch.cuda.synchronize()
    for k, lr in enumerate([1e-3, 1e-3, 5e-4, 2.5e-4]):
        _torch_step(ref, topt, grads[k], lr=lr)
    assert opt.step_count == 4
    d = _maxdiff(mine, ref)
    print('lr sequence through one captured step: max |param - torch| =', d)
    assert d < BAR
    assert opt.state_dict()['param_groups'][0]['lr'] == 2.5e-4
    assert opt.lr == 2.5e-4
    for g_ in opt.param_groups:     # the torch idiom
        g_['lr'] *= 0.5
    assert opt.lr == 1.25e-4


# ------------------------------------------------------------------------------------------------ 3. lr = 0
def test_zero_learning_rate_leaves_parameters_bit_unchanged():
    ps, ref, topt, mine, opt, grads = _make(lr=1e-3)
    st = _Stepper(opt)
    st.load(grads[0])
    st.capture()
    st.replay(grads[0])
    opt.lr = 0.0
    torch.cuda.synchronize()
    p_before, m_before, steps = opt.flat_p.clone(), opt.exp_avg.clone(), opt.step_count
    st.replay(grads[1])
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_p, p_before)
    assert not torch.equal(opt.exp_avg, m_before)
    assert opt.step_count == steps + 1 == 2


def test_zero_learning_rate_from_a_schedule_freezes_a_graphed_mf_step():
    """end to end: the captured DIS-MF step (construction of tests/test_determinism_gpu.py) driven through trainer.LRSchedule"""
    from depthinspace_amd import synth
    from depthinspace_amd.model import multi_frame_networks, multi_frame_worker
    from depthinspace_amd.trainer import FlatAdam, GraphedStep, LRSchedule
    H = W = 64
    settings = synth.make_settings(H, W)
    torch.manual_seed(0)
    args = argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic',
                              architecture='multi_frame', epochs=1, warmup_epochs=150, train_batch_size=1, max_disp=128)
    w = multi_frame_worker.Worker(args, settings=settings)
    net = multi_frame_networks.FuseNet((H, W), settings.K, settings.baseline).cuda()
    w.build_losses()
    w.current_epoch = 2
    opt = FlatAdam(net.parameters(), lr=1e-4)
    sched = LRSchedule(opt, lambda epoch: 1.0 if epoch < 1 else 0.0)
    batch = {k: torch.from_numpy(v) for k, v in synth.make_batch(settings, 1, 4, seed=4321, scene='bumps').items()}
    gs = GraphedStep(w, net, opt, batch, use_graph=True, warmup=1, strict=True)
    p0 = opt.flat_p.clone()
    gs.run()
    gs.run()
    torch.cuda.synchronize()
    assert gs.mode == 'graph' and opt.step_count == 2
    assert not torch.equal(opt.flat_p, p0)          # (lr 1e-4: the first two replays train)
    graphs = gs._graphs
    sched.step()
    assert opt.lr == 0.0 and sched.get_last_lr() == [0.0]
    p_before, m_before = opt.flat_p.clone(), opt.exp_avg.clone()
    gs.run()
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_p, p_before)
    assert not torch.equal(opt.exp_avg, m_before)
    assert opt.step_count == 3
    assert gs.mode == 'graph' and gs._graphs is graphs   # no re-capture


# ------------------------------------------------------------------------------------------------ 4. clipping
@pytest.mark.parametrize('graphed', [False, True])
def test_clipping_equals_torch(graphed):
    """gradient norms ~18, 1.8, 0.18, 0.018 (329 normal entries scaled by 10^-k) against max_grad_norm 0.5: two clipped steps,
    two unclipped, then max_grad_norm lowered to 1e-3 between steps: clipped again"""
    max_norm = 0.5
    ps, ref, topt, mine, opt, grads = _make(lr=1e-3, max_grad_norm=max_norm)
    norms = [float(_flat(gr).double().norm()) for gr in grads]
    assert norms[1] > max_norm > norms[2]
    st = _Stepper(opt)
    if graphed:
        st.load(grads[0])
        st.capture()
    step = st.replay if graphed else st.eager
    for k in range(5):
        gr = grads[min(k, 3)]
        if k == 4:
            max_norm = 1e-3
            opt.max_grad_norm = max_norm
        step(gr)
        _torch_step(ref, topt, gr, max_norm=max_norm)
        nrm, coef = opt.last_grad_norm, opt.last_clip_coef
        ref_n = norms[min(k, 3)]
        print(k, 'norm', nrm, 'fp64', ref_n, 'coef', coef, 'max |param - torch|', _maxdiff(mine, ref))
        assert abs(nrm - ref_n) <= 1e-10 * ref_n      # n * 2^-53 at n < 1e6
        if k in (2, 3):
            assert coef == 1.0
        else:
            want = float(torch.tensor(max_norm, dtype=torch.float32)) / (ref_n + 1e-6)   # (max_norm is a float on the device)
            assert coef < 1.0 and abs(coef - want) <= 1e-9 * want
        assert _maxdiff(mine, ref) < BAR
    assert opt.step_count == 5 and opt.skipped_steps == 0


def test_clipping_is_turned_on_at_construction_only():
    ps, ref, topt, mine, opt, grads = _make(lr=1e-3)
    assert opt.mode == 0 and opt.max_grad_norm is None
    with pytest.raises(ValueError):
        opt.max_grad_norm = 1.0
    opt.param_groups[0]['max_grad_norm'] = 1.0      # behind the property's back: refused at the next step
    with pytest.raises(ValueError):
        opt.sync_hyper()
    ps, ref, topt, mine, opt, grads = _make(lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        opt.max_grad_norm = None
    opt.max_grad_norm = 2.0
    assert opt.max_grad_norm == 2.0 and opt.mode == 1


# ------------------------------------------------------------------------------------------------ 5. reproducible norm
@pytest.mark.parametrize('which', [0, 1, 2])
def test_norm_and_clipped_step_repeat_bit_for_bit(which):
    """two eager runs and one captured call replayed: statistics, parameters, moments and state torch.equal (clipping active:
    the coefficient, hence every updated value, depends on every bit of the norm)"""
    from depthinspace_amd import lib, ops
    count = _counts()[which]
    g = torch.Generator().manual_seed(20 + which)
    p0 = torch.randn(count, generator=g).cuda()
    gr = torch.randn(count, generator=g).cuda()
    hyper = torch.tensor([1e-3, 0.25, 0.0, 0.0], dtype=torch.float32).cuda()
    partials = torch.empty(lib.fn('dis_adam_step_hyper_workspace')(count), dtype=torch.float64, device='cuda')

    def fresh():
        return [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(4, dtype=torch.int32, device='cuda'),
                torch.zeros(4, dtype=torch.float64, device='cuda')]

    def call(t):
        ops.adam_step_hyper(t[0], gr, t[1], t[2], t[3], hyper, t[4], partials, 3)

    runs = []
    for _ in range(2):
        t = fresh()
        call(t)
        call(t)
        torch.cuda.synchronize()
        runs.append(t)
    t = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):
        call(t)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    runs.append(t)
    ref = float(gr.double().norm())
    assert abs(float(runs[0][4][0]) - ref) <= 1e-10 * ref and float(runs[0][4][1]) < 1.0
    assert int(runs[0][3][0]) == 2
    for other, what in ((runs[1], 'second eager run'), (runs[2], 'graph replay')):
        for a, b, name in zip(runs[0], other, ('param', 'exp_avg', 'exp_avg_sq', 'state', 'stats')):
            assert torch.equal(a, b), (count, what, name)


# ------------------------------------------------------------------------------------------------ 6. non-finite skip
def test_nonfinite_gradient_skips_the_step():
    ps, ref, topt, mine, opt, grads = _make(lr=1e-3, skip_nonfinite=True)
    assert opt.mode == 2
    st = _Stepper(opt)
    st.load(grads[0])
    st.capture()

    def bad_step(flat, step):
        torch.cuda.synchronize()
        before = [t.clone() for t in _tensors(opt)[:4]]
        skipped = opt.skipped_steps
        step(flat)
        torch.cuda.synchronize()
        for a, b, name in zip(before, _tensors(opt)[:4], ('param', 'exp_avg', 'exp_avg_sq', 'state')):
            assert torch.equal(a, b), name
        assert opt.skipped_steps == skipped + 1
        assert float(opt.stats_dev[3]) == 1.0

    st.eager(grads[0])
    nan_last = _flat(grads[1]).clone()
    nan_last[N - 1] = float('nan')
    bad_step(nan_last, st.eager)                    # NaN in the last real element, eager
    st.replay(grads[1])
    assert float(opt.stats_dev[3]) == 0.0
    inf_first = _flat(grads[2]).clone()
    inf_first[0] = float('inf')
    bad_step(inf_first, st.replay)                  # +inf in element 0, through the captured step
    st.eager(grads[2])
    torch.cuda.synchronize()
    for k in range(3):                              # a torch run that never saw the bad steps
        _torch_step(ref, topt, grads[k])
    d = _maxdiff(mine, ref)
    print('after 3 good + 2 skipped steps: max |param - torch| =', d)
    assert d < BAR
    assert opt.step_count == 3 == int(float(topt.state_dict()['state'][0]['step'])) and opt.skipped_steps == 2
    # 1e30 everywhere: finite, its square overflows fp32 but not the fp64 sums - not skipped
    huge = torch.full((N,), 1e30)
    st.replay(huge)
    torch.cuda.synchronize()
    ref_n = float(huge.double().norm())
    assert opt.step_count == 4 and opt.skipped_steps == 2 and float(opt.stats_dev[3]) == 0.0
    assert abs(opt.last_grad_norm - ref_n) <= 1e-10 * ref_n


# ------------------------------------------------------------------------------------------------ 7. state round trip
def test_state_round_trip_restores_clipping_and_uploads_lr():
    from depthinspace_amd.trainer import FlatAdam, LRSchedule, step_decay
    ps, ref, topt, mine, a, grads = _make(lr=3e-4, max_grad_norm=2.0, skip_nonfinite=True)
    sa = _Stepper(a)
    sa.eager(grads[0])
    sd = a.state_dict()
    g0 = sd['param_groups'][0]
    assert g0['lr'] == 3e-4 and g0['max_grad_norm'] == 2.0 and g0['skip_nonfinite'] is True
    b = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in mine])      # defaults: lr 1e-4, mode 0
    assert b.mode == 0
    b.load_state_dict(sd)
    assert b.mode == 3 and b.max_grad_norm == 2.0 and b.skip_nonfinite and b.lr == 3e-4 and b.step_count == 1
    sb = _Stepper(b)
    sa.eager(grads[0])      # norm ~18 > 2: clipped
    sb.eager(grads[0])
    torch.cuda.synchronize()
    assert a.last_clip_coef < 1.0
    for x, y, name in zip(_tensors(a), _tensors(b), ('param', 'exp_avg', 'exp_avg_sq', 'state', 'stats')):
        assert torch.equal(x, y), name
    # torch.optim.Adam's own state (no max_grad_norm / skip_nonfinite keys) still loads and leaves the settings alone
    _torch_step(ref, topt, grads[0])
    tsd = topt.state_dict()
    assert 'max_grad_norm' not in tsd['param_groups'][0]
    c = FlatAdam([torch.nn.Parameter(p.clone().cuda()) for p in ps], max_grad_norm=2.0)
    c.load_state_dict(tsd)
    assert c.mode == 1 and c.max_grad_norm == 2.0 and c.lr == 3e-4 and c.step_count == 1
    d = FlatAdam([torch.nn.Parameter(p.clone().cuda()) for p in ps])
    d.load_state_dict(tsd)
    assert d.mode == 0 and d.step_count == 1
    assert not {'max_grad_norm', 'skip_nonfinite'} & set(d.state_dict()['param_groups'][0])
    # the schedule: a restored one gives the same next learning rate
    s1 = LRSchedule(a, step_decay(2, 0.5))
    for _ in range(3):
        s1.step()
    s2 = LRSchedule(b, step_decay(2, 0.5))
    s2.load_state_dict(s1.state_dict())
    s1.step()
    s2.step()
    assert a.lr == b.lr == s1.get_last_lr()[0] == s2.get_last_lr()[0] == 3e-4 * 0.25


# ------------------------------------------------------------------------------------------------ Worker.train and the schedule
def test_worker_saves_and_resumes_the_schedule(tmp_path):
    """Worker.do(..., scheduler=) at 64 x 64: the checkpoint holds the scheduler and the learning rate of the epoch a resumed run
    starts with, the resumed epoch trains at that rate, and the clip figures are logged beside the loss"""
    import os
    import numpy as np
    from depthinspace_amd import synth
    from depthinspace_amd.data import dataset as D
    from depthinspace_amd.model import networks, single_frame_worker
    from depthinspace_amd.trainer import FlatAdam, LRSchedule, step_decay
    settings = synth.make_settings(64, 64)
    root = str(tmp_path / 'data')
    D.write_synthetic_dataset(root, settings, 6, seed=50)
    mk = dict(data_root=root, output_dir=str(tmp_path / 'out'), num_workers=0, test_batch_size=1)

    def build(epochs):
        args = argparse.Namespace(use_pseudo_gt=False, lcn_radius=5, track_length=4, data_type='synthetic',
                                  architecture='single_frame', epochs=epochs, warmup_epochs=150, train_batch_size=2, max_disp=128)
        w = single_frame_worker.Worker(args, **mk)
        net = networks.DispDecoder(channels_in=2, max_disp=128, imsizes=w.imsizes).cuda()
        opt = FlatAdam(net.parameters(), lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
        return w, net, opt, LRSchedule(opt, step_decay(1, 0.5))

    w, net, opt, sched = build(2)
    w.do(net, opt, cmd='retrain', scheduler=sched)
    exp = os.path.join(str(tmp_path / 'out'), 'single_frame')
    lines = [ln for ln in open(os.path.join(exp, 'train.log')) if 'train e' in ln and 'loss=' in ln]   # (the worker's own log file)
    assert len(lines) == 4 and all('grad_norm=' in ln and 'skipped=0' in ln for ln in lines)
    assert opt.step_count == 4 and opt.lr == 1e-4 * 0.25            # 2 epochs x (4 train tracks / bs 2); two scheduler steps
    assert float(opt.hyper_dev[0]) == float(np.float32(1e-4 * 0.5))   # epoch 1 trained at half the rate
    state = torch.load(os.path.join(exp, 'state.dict'), weights_only=False)
    assert state['scheduler']['last_epoch'] == 2 and state['epoch'] == 1
    g0 = state['optimizer']['param_groups'][0]
    assert g0['lr'] == 1e-4 * 0.25 and g0['max_grad_norm'] == 1.0 and g0['skip_nonfinite'] is True
    w2, net2, opt2, sched2 = build(3)
    w2.do(net2, opt2, cmd='resume', scheduler=sched2)
    assert opt2.step_count == 6 and sched2.last_epoch == 3
    assert float(opt2.hyper_dev[0]) == float(np.float32(1e-4 * 0.25))  # epoch 2 trained at the restored rate
    assert opt2.lr == 1e-4 * 0.125 and opt2.skipped_steps == 0
