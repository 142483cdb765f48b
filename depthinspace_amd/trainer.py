"""Optimiser and data-parallel plumbing of the step: one flat fp32 parameter / gradient buffer, a fused Adam kernel over
it (dis_adam_step_hyper: step counter, learning rate and the clip / skip decision on the device, so a captured step replays
correctly and honours a learning rate changed between replays), a LambdaLR-style schedule, and the gradient all-reduce over
RCCL (torch.distributed 'nccl'), bucketed and overlapped with the backward pass.

The reference uses torch.optim.Adam(lr=1e-4) on a single GPU (train_val.py:55-56) and has no communication layer; data
parallelism here is batch sharding with mean-of-per-rank gradients: rank r owns its own tracks,
every rank holds full replicas of the parameters and of the Adam state.
"""
import contextlib
import gc
import os

import torch

from . import ops


@contextlib.contextmanager
def no_gc():
    """Collect now, then keep Python's cyclic collector off for the block.  For stream captures: torch.cuda.graph no longer collects
    on entry (torch >= 2.9), and a torch.cuda.CUDAGraph that a dead reference cycle still holds may be destroyed by a collection
    that happens to start INSIDE another capture.  On ROCm its destructor synchronises the device, which a capture in progress
    forbids; the error is thrown from a destructor and the process aborts.  Whether it happens depends only on how many
    objects the process allocated before (the collector's counters): an unrelated change moves it."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


@contextlib.contextmanager
def graph_capture(graph, **kwargs):
    """torch.cuda.graph(graph, **kwargs) with no finaliser running inside the capture (no_gc)"""
    with no_gc():
        with torch.cuda.graph(graph, **kwargs):
            yield


def init_distributed(backend=None):
    """Join the process group torchrun describes (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*) and bind this process to its
    GPU.  Call it BEFORE the first HIP call of the process.  Returns (rank, world_size, local_rank); (0, 1, 0) and no process
    group when the process was not started by a launcher."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')  # the host driver only supports dmabuf IPC
        if torch.cuda.device_count() > 0:
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        if not torch.distributed.is_initialized():
            torch.distributed.init_process_group(backend or os.environ.get('DIS_DIST_BACKEND', 'nccl'), rank=rank,
                                                 world_size=world)
    return rank, world, local_rank


class AbiComm(object):
    """The C ABI's own gradient exchange (include/dis_hip.h: dis_allreduce_*; RCCL bound by the library itself) - what a host
    that is not PyTorch would use.  torch.distributed (any backend) only carries rank 0's 128-byte id to the other ranks.
    FlatAdam uses it instead of torch.distributed.all_reduce when DIS_ALLREDUCE=abi."""

    def __init__(self, rank=0, world_size=1, process_group=None, unique_id=None):
        import ctypes
        L = ops.lib
        self._ct = ctypes
        self.rank, self.world_size = rank, world_size
        if unique_id is None:
            buf = ctypes.create_string_buffer(128)
            if rank == 0:
                rc = L.fn('dis_allreduce_unique_id')(ctypes.cast(buf, ctypes.c_void_p))
                if rc != 0:
                    raise L.DisHipError(f'dis_allreduce_unique_id failed: {rc}')
            obj = [buf.raw]
            if world_size > 1:
                torch.distributed.broadcast_object_list(obj, src=0, group=process_group)
            unique_id = obj[0]
        assert len(unique_id) == 128
        self.unique_id = bytes(unique_id)
        idb = ctypes.create_string_buffer(self.unique_id, 128)
        h = ctypes.c_void_p()
        rc = L.fn('dis_allreduce_init')(ctypes.cast(ctypes.pointer(h), ctypes.c_void_p), ctypes.cast(idb, ctypes.c_void_p), world_size, rank)
        if rc != 0:
            raise L.DisHipError(f'dis_allreduce_init failed: {rc}')
        self.handle = h

    def all_reduce(self, t, average=False):
        """in place on a contiguous fp32 device tensor, asynchronous on the current stream"""
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        ops.lib.call('dis_allreduce_sum_f32', self.handle.value, t, t.numel(), 1 if average else 0)

    def close(self):
        if self.handle is not None and self.handle.value:
            ops.lib.fn('dis_allreduce_destroy')(self.handle)
            self.handle = None


class _Done(object):
    def wait(self):
        pass


class FlatAdam(object):
    """Adam with torch.optim.Adam's default hyper-parameters on a flattened view of `params`.

    All parameters (also the never-used `upconv1/2` of FuseNet, whose gradient stays zero: a zero gradient leaves an Adam
    parameter unchanged) are re-pointed into one contiguous buffer; gradients are accumulated by autograd - or written by
    the weight-gradient kernels themselves (ops._sink) - directly into the matching views of one flat gradient buffer.

    Data parallelism (world_size > 1): the flat gradient is cut into buckets of ~`bucket_mb` in REVERSE parameter order
    (the order the backward pass completes them).  Every finished parameter gradient notifies its bucket (ops._sink for the
    kernels that write the flat buffer, a post-accumulate hook for gradients autograd adds); a complete bucket is
    all-reduced at once on a communication stream while the backward pass goes on.  How many notifications complete a
    parameter is learnt in the first step (which reduces everything after backward, like overlap=False); a later step
    that notifies differently fails loudly.  step() waits for the collectives and runs the fused Adam kernel with
    grad_scale = 1/world_size (mean of the per-rank gradients).  Inside a hipGraph capture the hooks stay silent: the
    caller places all_reduce_grads() between captured segments (bench.py).

    Hyper-parameters live in `param_groups[0]` (a real dict, torch.optim's layout: `for g in opt.param_groups: g['lr'] *= 0.5`
    works, and so does `opt.lr = x`) and are mirrored in `hyper_dev`, which the kernel reads: sync_hyper() uploads them when
    they changed, so a captured step follows a scheduler without re-capture.
    max_grad_norm: clip by global L2 norm (torch.nn.utils.clip_grad_norm_; with world_size > 1 the norm of the MEAN gradient,
    taken after the all-reduce, so every rank decides alike).  skip_nonfinite: a step whose gradient norm is inf / NaN changes
    nothing and is counted.  Both are decided on the device.  Which of the two are on (`mode`) is fixed at construction - it
    decides which kernels a captured step contains; the VALUE of max_grad_norm may change at any time."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, world_size=None, process_group=None,
                 bucket_mb=16.0, overlap=True, max_grad_norm=None, skip_nonfinite=False):
        self.params = [p for p in params]
        assert len(self.params) > 0
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.n = n
        pad = (n + 3) // 4 * 4
        self.flat_p = torch.zeros(pad, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(pad, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(pad, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(pad, dtype=torch.float32, device=dev)
        # {int steps taken, float 1-beta1^t, float sqrt(1-beta2^t), unused}: advanced by dis_adam_step_dev on the device
        self.state_dev = torch.zeros(4, dtype=torch.int32, device=dev)
        # {lr, max_norm, reserved, reserved}: what the kernel reads; written by sync_hyper() only
        self.hyper_dev = torch.zeros(4, dtype=torch.float32, device=dev)
        # {gradient norm, clip coefficient, skipped steps, skipped the last step}: written by the kernel when mode != 0
        self.stats_dev = torch.zeros(4, dtype=torch.float64, device=dev)
        self.stats_dev[1] = 1.0
        self.offsets = []
        off = 0
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                self.flat_p[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[off:off + k].view(p.shape)
                p.grad = self.flat_g[off:off + k].view(p.shape)
                self.offsets.append(off)
                off += k
        self.param_groups = [{'lr': lr, 'betas': tuple(betas), 'eps': eps, 'weight_decay': 0, 'amsgrad': False,
                              'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False,
                              'fused': None, 'max_grad_norm': None if max_grad_norm is None else float(max_grad_norm),
                              'skip_nonfinite': bool(skip_nonfinite), 'params': list(range(len(self.params)))}]
        self._uploaded = None      # (lr, max_norm) as last written to hyper_dev
        self.partials = None
        self._set_mode((1 if max_grad_norm is not None else 0) | (2 if skip_nonfinite else 0))
        if world_size is None:
            world_size = torch.distributed.get_world_size(process_group) if torch.distributed.is_initialized() else 1
        self.world_size = world_size
        self.process_group = process_group
        self.overlap = bool(overlap) and world_size > 1
        # DIS_ALLREDUCE=abi: the exchange goes through the C ABI's dis_allreduce_* (the library's own RCCL binding) instead of
        # torch.distributed.all_reduce - same buckets, same streams
        self._abi = None
        if world_size > 1 and dev.type == 'cuda' and os.environ.get('DIS_ALLREDUCE', '') == 'abi':
            self._abi = AbiComm(torch.distributed.get_rank(process_group), world_size, process_group)
        if dev.type == 'cuda':
            ops.register_grad_sinks(self.params, self._notify if self.overlap else None)
        # ---- buckets (reverse parameter order)
        self.buckets = []          # [lo, hi) ranges of the flat buffer, in the order the backward pass finishes them
        self._bucket_of = {}       # param index -> bucket index
        if self.overlap:
            limit = int(bucket_mb * (1 << 20) / 4)
            hi = n
            cur = []
            for i in range(len(self.params) - 1, -1, -1):
                cur.append(i)
                lo = self.offsets[i]
                if hi - lo >= limit or i == 0:
                    for j in cur:
                        self._bucket_of[j] = len(self.buckets)
                    self.buckets.append((lo, hi))
                    hi, cur = lo, []
            self._index = {id(p): i for i, p in enumerate(self.params)}
            self._expected = None                      # notifications per parameter, learnt in the first step
            self._seen = [0] * len(self.params)
            self._works = []
            self._reduced = [False] * len(self.buckets)
            self._comm_stream = torch.cuda.Stream(device=dev) if dev.type == 'cuda' else None
            for p in self.params:
                p.register_post_accumulate_grad_hook(self._notify)

    # ------------------------------------------------------------------ gradient notifications -> bucketed all-reduce
    def _notify(self, p):
        if not self.overlap or (self.flat_g.is_cuda and torch.cuda.is_current_stream_capturing()):
            return
        i = self._index.get(id(p))
        if i is None:
            return
        self._seen[i] += 1
        if self._expected is None:
            return  # calibration step
        if self._seen[i] > self._expected[i]:
            raise RuntimeError(f'FlatAdam: parameter {i} received more gradient contributions than in the first step; '
                               f'the overlapped all-reduce needs a static graph (use overlap=False)')
        if self._seen[i] == self._expected[i]:
            b = self._bucket_of[i]
            self._pending[b] -= 1
            if self._pending[b] == 0:
                self._reduce_bucket(b)

    def _reduce_bucket(self, b):
        lo, hi = self.buckets[b]
        view = self.flat_g[lo:hi]
        if self._comm_stream is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self._comm_stream.wait_event(ev)
            with torch.cuda.stream(self._comm_stream):
                if self._abi is not None:
                    self._abi.all_reduce(view)
                    w = _Done()
                else:
                    w = torch.distributed.all_reduce(view, group=self.process_group, async_op=True)
        else:
            w = torch.distributed.all_reduce(view, group=self.process_group, async_op=True)
        self._works.append(w)
        self._reduced[b] = True

    def _arm(self):
        if not self.overlap:
            return
        self._seen = [0] * len(self.params)
        self._works = []
        self._reduced = [False] * len(self.buckets)
        if self._expected is not None:
            self._pending = [0] * len(self.buckets)
            for i, e in enumerate(self._expected):
                if e > 0:
                    self._pending[self._bucket_of[i]] += 1

    def finish_grads(self):
        """every bucket reduced (SUM over ranks) and visible to the current stream"""
        if self.world_size <= 1:
            return
        if not self.overlap or (self.flat_g.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.all_reduce_grads()
            return
        if self._expected is None:
            self._expected = list(self._seen)   # first step: learn, reduce everything now
            self.all_reduce_grads()
            return
        for i, (s, e) in enumerate(zip(self._seen, self._expected)):
            if s != e:
                raise RuntimeError(f'FlatAdam: parameter {i} got {s} gradient contributions, {e} in the first step')
        for b in range(len(self.buckets)):
            if not self._reduced[b]:      # buckets of parameters that never receive a gradient (upconv1/2): zeros
                self._reduce_bucket(b)
        if self._comm_stream is not None:
            with torch.cuda.stream(self._comm_stream):
                for w in self._works:
                    w.wait()
            torch.cuda.current_stream().wait_stream(self._comm_stream)
        else:
            for w in self._works:
                w.wait()
        self._works = []

    # ------------------------------------------------------------------ torch.optim-like surface
    def zero_grad(self, set_to_none=False):
        self.flat_g.zero_()
        ops.reset_grad_sinks()
        if self.flat_g.is_cuda:
            ops.begin_step(self.flat_g.device)
        self._arm()

    def all_reduce_grads(self):
        if self.world_size > 1:
            if self._abi is not None:
                self._abi.all_reduce(self.flat_g)
            else:
                torch.distributed.all_reduce(self.flat_g, group=self.process_group)

    @property
    def step_count(self):
        return int(self.state_dev[0])  # device -> host: only checkpointing / tests read it

    # ------------------------------------------------------------------ hyper-parameters: host dict <-> hyper_dev
    def _set_mode(self, mode):
        self.mode = mode
        if mode != 0 and self.partials is None:
            k = ops.lib.fn('dis_adam_step_hyper_workspace')(self.flat_p.numel())
            if k < 0:
                raise RuntimeError(f'FlatAdam: no gradient-norm kernel for {self.flat_p.numel()} parameters')
            self.partials = torch.empty(k, dtype=torch.float64, device=self.flat_p.device)

    lr = property(lambda self: self.param_groups[0]['lr'],
                  lambda self, v: self.param_groups[0].__setitem__('lr', v))
    betas = property(lambda self: self.param_groups[0]['betas'],
                     lambda self, v: self.param_groups[0].__setitem__('betas', tuple(v)))
    eps = property(lambda self: self.param_groups[0]['eps'],
                   lambda self, v: self.param_groups[0].__setitem__('eps', v))
    skip_nonfinite = property(lambda self: bool(self.mode & 2))

    @property
    def max_grad_norm(self):
        return self.param_groups[0]['max_grad_norm']

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        if (v is None) != (not self.mode & 1):
            raise ValueError('FlatAdam: clipping is turned on or off at construction (it decides which kernels a captured '
                             'step contains); only the value of max_grad_norm can change later')
        self.param_groups[0]['max_grad_norm'] = None if v is None else float(v)

    def _host_hyper(self):
        g = self.param_groups[0]
        mn = g.get('max_grad_norm')
        if (mn is None) != (not self.mode & 1) or bool(g.get('skip_nonfinite', False)) != bool(self.mode & 2):
            raise ValueError('FlatAdam: max_grad_norm / skip_nonfinite were turned on or off after construction')
        return (float(g['lr']), 0.0 if mn is None else float(mn))

    def sync_hyper(self):
        """hyper_dev = the host's (lr, max_norm) if they changed since the last upload: a stream-ordered copy on the current
        stream, nothing otherwise.  Issues nothing inside a capture and raises there if the device copy is stale."""
        want = self._host_hyper()
        if want == self._uploaded:
            return
        if self.hyper_dev.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FlatAdam: hyper-parameters changed inside a capture; call sync_hyper() before capturing')
        self._hyper_host = torch.tensor([want[0], want[1], 0.0, 0.0], dtype=torch.float32)
        self.hyper_dev.copy_(self._hyper_host, non_blocking=True)
        self._uploaded = want

    # for logging and tests only: each read is a device -> host synchronisation
    @property
    def last_grad_norm(self):
        """global L2 norm of the (mean) gradient of the last step (mode != 0)"""
        return float(self.stats_dev[0])

    @property
    def last_clip_coef(self):
        """clip coefficient of the last step (1.0: not clipped)"""
        return float(self.stats_dev[1])

    @property
    def skipped_steps(self):
        """number of steps skipped for a non-finite gradient so far"""
        return int(self.stats_dev[2])

    def step(self, all_reduce=True):
        # every GroupNorm token of this backward pass redeemed, every pre-reduced gradient picked up - checked BEFORE the update
        # (a stale table means gradients of this step are wrong; the next zero_grad() would be one update too late)
        ops.check_backward_complete()
        if all_reduce:
            self.finish_grads()
        self.sync_hyper()
        ops.adam_step_hyper(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.state_dev, self.hyper_dev,
                            self.stats_dev, self.partials, self.mode, self.betas[0], self.betas[1], self.eps,
                            1.0 / self.world_size)

    def broadcast_parameters(self, src=0):
        """identical replicas: parameters, moments, the step counter, the hyper-parameters and the clip / skip statistics of
        rank `src`"""
        if self.world_size > 1:
            g = self.param_groups[0]
            hyper = [g['lr'], g['max_grad_norm']]
            torch.distributed.broadcast_object_list(hyper, src=src, group=self.process_group)
            g['lr'] = hyper[0]
            if self.mode & 1:
                g['max_grad_norm'] = hyper[1]
            self.sync_hyper()
            for t in (self.flat_p, self.exp_avg, self.exp_avg_sq, self.state_dev, self.stats_dev):
                torch.distributed.broadcast(t, src, group=self.process_group)
            ops.params_changed()   # (weights packed by this step's batch launch are stale)

    # torch.optim.Adam's own (de)serialisation layout, so state.dict files are interchangeable with the reference's
    # (reference model/worker.py:342-364,376-402 saves optimizer.state_dict() of torch.optim.Adam)
    def state_dict(self):
        step = float(self.step_count)
        state = {}
        if step > 0:
            for i, (p, off) in enumerate(zip(self.params, self.offsets)):
                k = p.numel()
                state[i] = {'step': torch.tensor(step), 'exp_avg': self.exp_avg[off:off + k].view(p.shape).clone(),
                            'exp_avg_sq': self.exp_avg_sq[off:off + k].view(p.shape).clone()}
        group = dict(self.param_groups[0], betas=tuple(self.betas), params=list(range(len(self.params))))
        if self.mode == 0:   # (plain Adam: exactly torch.optim.Adam's keys)
            del group['max_grad_norm'], group['skip_nonfinite']
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        if 'param_groups' not in sd:  # round-1 private layout: {'step', 'exp_avg', 'exp_avg_sq'} flat
            self._set_step(int(sd['step']))
            self.exp_avg[:self.n].copy_(sd['exp_avg'])
            self.exp_avg_sq[:self.n].copy_(sd['exp_avg_sq'])
            return
        groups = sd['param_groups']
        ids = [i for g in groups for i in g['params']]
        if len(ids) != len(self.params):
            raise ValueError(f'optimizer state has {len(ids)} parameters, this model has {len(self.params)}')
        g0 = groups[0]
        if g0.get('amsgrad') or g0.get('weight_decay', 0) or g0.get('maximize'):
            raise ValueError('only plain Adam (no amsgrad / weight decay / maximize) is supported')
        self.lr, self.betas, self.eps = float(g0['lr']), tuple(g0['betas']), float(g0['eps'])
        # (sync_hyper() uploads the learning rate before the next step.)  Clipping / skipping as saved; a state without the keys
        # - torch.optim.Adam's, the reference's - leaves this optimiser's own settings alone
        if 'max_grad_norm' in g0 or 'skip_nonfinite' in g0:
            mn = g0.get('max_grad_norm')
            self.param_groups[0]['max_grad_norm'] = None if mn is None else float(mn)
            self.param_groups[0]['skip_nonfinite'] = bool(g0.get('skip_nonfinite', False))
            self._set_mode((1 if mn is not None else 0) | (2 if g0.get('skip_nonfinite', False) else 0))
        steps = set()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for pos, (p, off) in enumerate(zip(self.params, self.offsets)):
            st = sd['state'].get(ids[pos])
            if st is None:
                continue  # a parameter that never received a gradient (upconv1/2) has no state in torch.optim.Adam
            k = p.numel()
            if tuple(st['exp_avg'].shape) != tuple(p.shape):
                raise ValueError(f'optimizer state {ids[pos]}: shape {tuple(st["exp_avg"].shape)} != {tuple(p.shape)}')
            self.exp_avg[off:off + k].copy_(st['exp_avg'].reshape(-1))
            self.exp_avg_sq[off:off + k].copy_(st['exp_avg_sq'].reshape(-1))
            steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError(f'per-parameter step counts differ ({sorted(steps)}): not representable in the fused optimiser')
        self._set_step(steps.pop() if steps else 0)

    def _set_step(self, step):
        b1, b2 = self.betas
        st = torch.zeros(4, dtype=torch.int32)
        st[0] = int(step)
        st[1:3] = torch.tensor([1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5], dtype=torch.float32).view(torch.int32)
        self.state_dev.copy_(st)


class GraphedStep(object):
    """One training step of a stage worker (`copy_data` + LCN, net_forward, loss_forward, backward, gradient all-reduce,
    Adam: the body of the reference loop, model/worker.py:499-539) on static device buffers, eager or captured in hipGraphs
    and replayed per batch.  bench.py and Worker.train_epoch(use_graph=True) both run THIS object, so the benchmark times
    the product's own loop.

    use_graph=False: the eager step (what Worker.train_step does): with world_size > 1 FlatAdam's hooks all-reduce every
      gradient bucket on the communication stream while the backward pass is still running.
    use_graph=True, world_size == 1: one graph (forward, losses, backward, Adam).
    world_size > 1 always runs the eager form: it is the one whose collectives overlap the backward pass, and it costs
      nothing (at N = 1 the eager loop reaches the captured loop's frames/s, bench.py `eager_launch_frames_per_s`).
      Captured multi-rank forms (graph, all-reduce, Adam graph; and a two-graph backward with the tail bucket reduced
      underneath the second graph) were built in round 2 and REMOVED: DIS-MF's faulted on its second replay in the 2-rank
      test, and neither can be validated on RCCL with the single GPU of the development box.
    The set of loss terms may change with the epoch (epoch < 2 adds the L1 warm-up term, reference
    model/multi_frame_worker.py:160-165): key() changes and the step is re-captured.
    Batches are copied into static device buffers (run(batch)); `errs` of the last step are in `loss_buf[:nterms]`."""

    def __init__(self, worker, net, opt, example_batch, use_graph=True, warmup=2, strict=False):
        self.worker, self.net, self.opt = worker, net, opt
        self.strict = strict          # True: a failing capture raises instead of falling back to eager launches
        self.capture_error = None     # why the step runs eagerly although a graph was asked for
        self.dev = opt.flat_p.device
        # (type(example_batch): an AssembledBatch of the packed loader stays one, so that copy_data takes the buffers as they are)
        from .data.packed import AssembledBatch
        self.static = (AssembledBatch if isinstance(example_batch, AssembledBatch) else dict)(
            (k, torch.as_tensor(v).to(self.dev).contiguous().clone()) for k, v in example_batch.items())
        self.loss_buf = torch.zeros(32, device=self.dev)
        self.nterms = 0
        self.world = opt.world_size
        self.use_graph = bool(use_graph) and self.world == 1
        self.warmup = warmup
        self._key = None
        self._graphs = None
        self.mode = 'eager-overlap' if (self.world > 1 and opt.overlap) else 'eager'

    # ---- pieces of the step
    def key(self):
        w = self.worker
        return (w.current_epoch < 2, w.current_epoch < w.warmup_epochs and w.data_type == 'real')

    def _forward_loss(self):
        w = self.worker
        w.copy_data(self.static, device=self.dev, requires_grad=False, train=True)
        self.opt.zero_grad()
        flow = w.read_optical_flow(train=True)
        out = w.net_forward(self.net, flow)
        errs = w.loss_forward(out, True, flow)
        if isinstance(errs, dict):
            errs = errs['errs']
        if not isinstance(errs, (list, tuple)):
            errs = [errs]
        self.nterms = len(errs)
        wv = getattr(errs, 'weighted', None)   # (ops.LossTerms: the terms as one vector, their sum as one autograd node)
        self.loss_buf[:len(errs)].copy_(wv.detach() if wv is not None else torch.stack([e.detach() for e in errs]))
        tot = getattr(errs, 'total', None)
        return tot if tot is not None else sum(errs)

    def _eager(self):
        self._forward_loss().backward()
        self.opt.step()

    def _capture(self):
        opt = self.opt
        opt.sync_hyper()   # (the capture itself may not upload; replays follow the host values through run())
        # the warm-up steps (kernel attributes, allocator pools, autograd nodes on the capture-compatible stream) must not train:
        # parameters, moments, the step counter and the skipped-step count are put back afterwards, so a graphed run takes exactly
        # the steps an eager one does
        state = (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.state_dev, opt.stats_dev)
        snap = [t.clone() for t in state]
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, self.warmup)):
                self._eager()
            for t, c in zip(state, snap):
                t.copy_(c)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g1 = torch.cuda.CUDAGraph()
        with graph_capture(g1):
            self._forward_loss().backward()
            opt.step(all_reduce=False)
        self._graphs, self.mode = (g1,), 'graph'

    # ---- public
    def run(self, batch=None, packed=None):
        """batch: host (or device) tensors copied into the static buffers.  packed: a data.packed.PackedBatch - the current stream
        waits for its upload, ONE launch assembles it into the static buffers (outside the capture, in front of the replay) and its
        device slot is handed back to the loader behind that launch."""
        if batch is not None:
            for k, v in batch.items():
                self.static[k].copy_(torch.as_tensor(v), non_blocking=True)
        if packed is not None:
            packed.assemble(out=self.static)
        if not self.use_graph:
            self._eager()
            return
        key = (self.key(), self.opt.mode)   # (mode: which optimiser kernels the graph holds; load_state_dict may change it)
        if self._graphs is None or self._key != key:
            self._graphs, self._key = None, key
            try:
                self._capture()
            except Exception as e:  # pragma: no cover
                if self.strict:
                    raise
                import logging
                self.capture_error = f'{type(e).__name__}: {e}'
                logging.warning(f'[GraphedStep] hipGraph capture failed ({self.capture_error}); running eagerly')
                self.use_graph, self._graphs = False, None
                self.mode = 'eager (capture failed)'
                torch.cuda.synchronize()
                self._eager()
                return
        self.opt.sync_hyper()   # a learning rate / max_norm changed since the last replay: one small upload, no re-capture
        self._graphs[0].replay()

    def losses(self):
        return [float(v) for v in self.loss_buf[:self.nterms].cpu()]


class LRSchedule(object):
    """lr = base_lr * lr_lambda(epoch): torch.optim.lr_scheduler.LambdaLR's contract (construction is epoch 0; step() goes to the
    next epoch) on anything that has `param_groups` - FlatAdam, which torch's own schedulers refuse, or a torch optimiser.  It only
    edits `param_groups[...]['lr']`; FlatAdam uploads the value before its next step or replay (sync_hyper).  Worker.train calls
    step() after every epoch, like the reference (model/worker.py:404-405).  As with LambdaLR, the lambda itself is not saved."""

    def __init__(self, optimizer, lr_lambda, last_epoch=-1):
        self.optimizer = optimizer
        self.lr_lambda = lr_lambda
        if last_epoch == -1:
            self.base_lrs = [g['lr'] for g in optimizer.param_groups]
        else:   # resuming without a state_dict: the optimiser must carry the initial learning rate, as torch demands
            self.base_lrs = [g['initial_lr'] for g in optimizer.param_groups]
        self.last_epoch = last_epoch
        self.step()

    def step(self):
        self.last_epoch += 1
        self._last_lr = [b * self.lr_lambda(self.last_epoch) for b in self.base_lrs]
        for g, v in zip(self.optimizer.param_groups, self._last_lr):
            g['lr'] = v

    def get_last_lr(self):
        return list(self._last_lr)

    def state_dict(self):
        return {'last_epoch': self.last_epoch, 'base_lrs': list(self.base_lrs), '_last_lr': list(self._last_lr)}

    def load_state_dict(self, sd):
        self.last_epoch = int(sd['last_epoch'])
        self.base_lrs = list(sd['base_lrs'])
        self._last_lr = list(sd.get('_last_lr', [b * self.lr_lambda(self.last_epoch) for b in self.base_lrs]))


def step_decay(step_size, gamma):
    """lr_lambda of torch.optim.lr_scheduler.StepLR: the learning rate times `gamma` every `step_size` epochs"""
    step_size = int(step_size)
    if step_size <= 0:
        raise ValueError('step_decay: step_size must be positive')
    return lambda epoch: gamma ** (epoch // step_size)
