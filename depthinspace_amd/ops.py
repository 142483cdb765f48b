"""torch.autograd wrappers over the C ABI (include/dis_hip.h).

Each Function allocates outputs/workspaces with torch (the caller owns all memory), launches the HIP
kernels on the current stream through `lib.call`, and wires the hand-written backward kernels.
No ATen compute op is used for the arithmetic of the step; torch is memory + autograd tape only.
"""
import os as _os_env
import torch
from . import lib

ACT_NONE, ACT_SELU, ACT_RELU = 0, 1, 2
CONV_ACCUM = 0x100
PHOTO_TYPES = {'mse': 0, 'sad': 1, 'census_mse': 2, 'census_sad': 3}


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('depthinspace_amd ops need CUDA(HIP) tensors: the HIP path is the only path')
        if t.dtype != torch.float32:
            raise RuntimeError(f'expected float32, got {t.dtype}')
        if not t.is_contiguous():
            raise RuntimeError('expected a contiguous tensor')


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# the parts the wrappers of the track tools share (render_track ... tsdf_mesh, at the end of this file)
def _fin(v):
    return v == v and abs(v) < float('inf')


def _k4(K):
    """fx, fy, cx, cy of the 3 x 3 host intrinsics K (numpy or a CPU tensor), as floats"""
    return [float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])]


def _workspace(name, need, workspace, dev):
    """a fresh workspace of `need` bytes, or the caller's once it is a contiguous uint8 device tensor (else RuntimeError) of at
    least `need` bytes at a 16-byte boundary (else DisHipError)"""
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise RuntimeError(f'{name}: workspace must be a contiguous uint8 CUDA(HIP) tensor')
    if workspace.numel() < need or workspace.data_ptr() % 16:
        raise lib.DisHipError(f'{name}: workspace must hold at least {need} bytes and be 16-byte aligned')
    return workspace


def _out_struct(cls, tensors):
    """the ctypes out-struct `cls` with the address of tensors[field] in every field; NULL for a field without a tensor, or with an
    empty one"""
    O = cls()
    for f, _ in cls._fields_:
        setattr(O, f, (tensors[f].data_ptr() or None) if f in tensors else None)
    return O


def _track_dims(name, x, what='disp', verb='is'):
    """n, tl, H, W of the maps x (n, tl, H, W) or (n, tl, 1, H, W)"""
    if not (x.dim() == 4 or (x.dim() == 5 and x.shape[2] == 1)):
        raise RuntimeError(f'{name}: {what} (n, tl, H, W) or (n, tl, 1, H, W) {verb} expected')
    return int(x.shape[0]), int(x.shape[1]), int(x.shape[-2]), int(x.shape[-1])


# Zeroed fp64 accumulators (GroupNorm statistics, loss sums) come from one arena per device that is cleared ONCE per
# step (begin_step, called by FlatAdam.zero_grad) instead of one tiny fill kernel per accumulator (~100 per step).
# A slice is handed out at most once between two clears; without begin_step (tests, inference) the arena simply runs
# out and plain torch.zeros takes over.
_ARENA = {}
_ARENA_DOUBLES = int(_os_env.environ.get('DIS_ARENA_DOUBLES', 3 << 22))   # 96 MiB (64 MiB sent 7 requests per DIS-MF step to torch.zeros): the per-workgroup channel-sum slots of the GroupNorm backward are 2 MiB per launch, ~30 per step


# gradient tensors whose producer already left the GroupNorm-backward sums (see _Conv2d.backward / _GroupNorm.backward):
# data_ptr -> (ab, slots)
_GN_PRE = {}
# GroupNorm backward applied ON LOAD by the input-gradient launch of the conv in front of the GroupNorm (round 5,
# dis_conv2d_dgrad_f16x2_gnb): the GroupNorm's backward runs only the coefficient kernel and returns a TOKEN in place of the gradient
# wrt its input - a one-element tensor expanded to the gradient's shape (no memory, an address no other tensor has); the conv's
# backward finds (g, q, coef, in_act) under the token's address.  token data_ptr -> (token, g, q, coef, in_act).  Only conv outputs
# that conv2d() / conv2d_gn_in() marked `_gn_lazy_ok` (their backward understands tokens, and the GroupNorm is their only consumer)
# are answered with one; begin_step() raises if a token was never redeemed.
_GN_LAZY = {}
GN_LAZY = _os_env.environ.get('DIS_GN_LAZY', '1') != '0'


# Forward twin of the tokens (round 5, dis_conv2d_fwd_f16x2_gnres): group_norm(..., residual, act=SELU, defer=True) does NOT run its
# elementwise pass; the output tensor exists but is unwritten, `_pending_gn` = (x2, stats, gamma, beta, residual, eps) hangs on it, and
# the 3x3 conv that consumes it first - conv2d() looks for the attribute - forms the values on load and stores them as a side
# output.  Every other reader must come after that conv (a ResNetBlock's own residual use does) or call realize() first;
# begin_step() raises if an output was never written.
_GN_PENDING = {}


def realize(t):
    """run the deferred GroupNorm pass of `t` now (a consumer without an on-load form)"""
    pend = getattr(t, '_pending_gn', None)
    if pend is not None:
        x2, stats, gamma, beta, res, eps = pend
        n, c = x2.shape[0], x2.shape[-1]
        lib.call('dis_gn_apply', x2, stats, gamma, beta, res, t, n, x2.numel() // (n * c), c, ACT_SELU, float(eps))
        t._pending_gn = None
        _GN_PENDING.pop(t.data_ptr(), None)
    return t


# Tokens come from a persistent per-device pool filled with NaN ONCE (unique addresses, no launch per step): arithmetic on a token
# that was not redeemed - autograd summing it with the gradient of a second consumer of the conv output - poisons the loss of the
# same step visibly.  _GN_TOKEN_FOR: uid of the conv node whose output a token stands for -> the token's address; that conv's
# backward raises if what it receives is not the token (see _gn_lazy_pop).
_TOKEN_POOL = {}
_TOKEN_POOL_SIZE = 4096
_GN_TOKEN_FOR = {}
import itertools as _it
_LAZY_UID = _it.count(1)


def _new_token(dev):
    pool = _TOKEN_POOL.get(dev)
    if pool is None:
        pool = _TOKEN_POOL[dev] = [torch.full((_TOKEN_POOL_SIZE,), float('nan'), dtype=torch.float32, device=dev), 0]
    if pool[1] >= _TOKEN_POOL_SIZE:   # (no begin_step between many backward passes: tests, ad-hoc use)
        return torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    i = pool[1]
    pool[1] = i + 1
    return pool[0][i:i + 1]


def _mark_lazy_ok(out):
    """`out` = (y, stats) of a conv node whose backward redeems GroupNorm tokens: a GroupNorm that is y's ONLY consumer may answer
    with one.  The mark is the node's uid (truthy); the node keeps it (the ctx of a torch.autograd.Function IS the output's grad_fn)."""
    uid = next(_LAZY_UID)
    out[0]._gn_lazy_ok = uid
    if out[0].grad_fn is not None:
        out[0].grad_fn.lazy_uid = uid


def _gn_coef(n, c, device):
    """the per-(sample, channel) coefficients of a GroupNorm backward formed from channel sums (dis_gn_bwd_coef / _from_sums)"""
    return torch.empty(n * (c + 2) + 4 * n * c + 2, dtype=torch.float32, device=device)


def _gn_sums(n, c, device, slots=None):
    """-> (ab, slots): zeroed per-workgroup slots for the GroupNorm-backward channel sums an input-gradient epilogue leaves"""
    slots = lib.fn('dis_conv2d_gnsums_slots')() if slots is None else int(slots)
    return _zeros_d(n * slots * 2 * c, device), slots


def _gn_lazy_defer(g, q, stats, gamma, ab, slots, gg, gb, n, hw, c, eps, in_act, uid=0):
    coef = _gn_coef(n, c, g.device)
    lib.call('dis_gn_bwd_coef', stats, gamma, ab, slots, coef, gg, gb, _zeros_d(1, g.device), n, hw, c, eps)
    tok = _new_token(g.device)
    _GN_LAZY[tok.data_ptr()] = (tok, g, q, coef, in_act)
    if uid and uid is not True:
        _GN_TOKEN_FOR[uid] = tok.data_ptr()
    return tok.expand(g.shape)


def _gn_lazy_pop(gy, ctx=None):
    ent = _GN_LAZY.pop(gy.data_ptr(), None) if _GN_LAZY else None
    if _GN_TOKEN_FOR:
        exp = _GN_TOKEN_FOR.pop(getattr(ctx, 'lazy_uid', None), None)
        if exp is not None and (ent is None or ent[0].data_ptr() != exp):
            if ent is not None:
                _GN_LAZY[gy.data_ptr()] = ent
            raise RuntimeError('ops: GroupNorm token was summed with another gradient: the conv output has a second consumer '
                               '(only an output whose ONLY consumer is the GroupNorm may be answered with a token)')
    return ent


def check_forward_complete():
    """no deferred GroupNorm output (group_norm(defer=True)) is left unwritten: called at the end of FuseNet's forward"""
    if _GN_PENDING:
        _GN_PENDING.clear()
        raise RuntimeError('ops: a deferred GroupNorm output (group_norm(defer=True)) of this forward pass was never realised')


def check_backward_complete():
    """every token redeemed, every pre-reduced gradient picked up: called by FlatAdam.step() BEFORE the update (and by tests)"""
    if _GN_LAZY or _GN_TOKEN_FOR:
        _GN_LAZY.clear()
        _GN_TOKEN_FOR.clear()
        raise RuntimeError('ops: a deferred GroupNorm backward (token gradient) of this backward pass was not redeemed')
    if _GN_PRE:
        _GN_PRE.clear()
        raise RuntimeError('ops: a pre-reduced GroupNorm gradient of this backward pass was not consumed')


def _gn_lazy_materialize(ent):
    """the elementwise pass as a launch of its own (the consumer has no on-load form for this configuration)"""
    _, g, q, coef, in_act = ent
    n, c = g.shape[0], g.shape[-1]
    gx = torch.empty_like(g)
    lib.call('dis_gn_bwd_apply_coef', g, q, coef, gx, n, g.numel() // (n * c), c, in_act)
    return gx


def _gn_lazy_shape(cin, cout, k, stride, pad):
    return GN_LAZY and BF16X3 and cin == cout and cin in (16, 32) and k == 3 and stride == 1 and pad == 1


def _gn_lazy_k4s2(cin_pad, cin, cout, k, stride, pad):
    """FuseNet's 4 x 4 stride-2 down convolution (dis_conv2d_wgrad_k4s2_f16x2_gnb; DIS_F2_WGRAD_K4S2=0 keeps it on the fp32 kernel)"""
    return (GN_LAZY and BF16X3 and cin_pad == cin == 32 and cout == 32 and (k, stride, pad) == (4, 2, 1) and
            _os_env.environ.get('DIS_F2_WGRAD_K4S2', '1') != '0')


def begin_step(dev):
    if _GN_PRE:   # a gradient that was handed on pre-multiplied was never picked up by its GroupNorm: the step would be wrong
        _GN_PRE.clear()
        raise RuntimeError('ops: a pre-reduced GroupNorm gradient of the previous backward pass was not consumed')
    if _GN_PENDING:  # a deferred GroupNorm output was never written
        _GN_PENDING.clear()
        raise RuntimeError('ops: a deferred GroupNorm output (group_norm(defer=True)) of the previous forward pass was never realised')
    if _GN_LAZY or _GN_TOKEN_FOR:  # a token stood in for a gradient and nobody redeemed it (the conv output had a second consumer?)
        _GN_LAZY.clear()
        _GN_TOKEN_FOR.clear()
        raise RuntimeError('ops: a deferred GroupNorm backward (token gradient) of the previous backward pass was not redeemed')
    dev = torch.device(dev)
    if dev in _TOKEN_POOL:
        _TOKEN_POOL[dev][1] = 0
    a = _ARENA.get(dev)
    if a is None:
        a = _ARENA[dev] = [torch.zeros(_ARENA_DOUBLES, dtype=torch.float64, device=dev), 0, 0]
    elif a[2] > 0:
        a[0][:a[2]].zero_()   # only what was handed out since the last clear (the rest is still zero)
    a[1] = 0
    a[2] = 0
    _PackBatch.begin_step(dev)


class _PackBatch(object):
    """One weight-packing launch per training step for the bf16 DispNetS path (dis_convb_pack_record / dis_convb_pack_batch).
    Every dis_convb_run call packs its fp32 weights into its `wpack` workspace first (~100 launches of 5 - 7 us per step).  The packed
    form depends on the weights alone, and those change once per step, so: the call sites keep PERSISTENT workspaces (keyed by
    weight address and call geometry); the first begin_step() outside a graph capture starts a record, the next one stops it, uploads
    the descriptors and from then on every begin_step() (FlatAdam.zero_grad, i.e. in front of the forward pass) packs ALL recorded
    calls in one launch; the calls then pass DIS_CONVB_PREPACKED.  Calls that were not in the record (another network, inference
    without begin_step) keep packing for themselves.  DIS_PACK_BATCH=0 disables it.

    Lifetime rules (the descriptor table holds RAW device pointers of the weights and of the workspaces):
      * every recorded entry holds a weak reference to its weight tensor; when one dies (the network was freed) the table is dropped
        before the next launch and recording starts over (`invalidate`); a weight that was a temporary copy while recording (it
        died although its network lives) switches the batching off for the process - its pointer can never be replayed;
      * a recorded workspace is never freed while the table exists: a size / device change of a recorded entry drops the table and
        parks the old buffer in `retired` (a captured hipGraph may still replay the launch that writes it);
      * an entry counts as prepacked only while its weight is the recorded tensor at the recorded `_version` (torch-side writes:
        copy_, load_state_dict, broadcast) and no parameter update ran since the batch launch (`params_changed`, called by the
        Adam entry points and by every FlatAdam method that rewrites the parameters);
      * entries that are not part of the table are evicted when the cache passes 4 * CAP entries."""
    enabled = _os_env.environ.get('DIS_PACK_BATCH', '1') != '0'
    CAP = 1024
    cache = {}        # key -> [wpack tensor, in_table, weakref(weight), weight._version at the last batch launch]
    state = 'idle'    # idle -> recording -> ready   (off: more calls than the table holds / an unstable weight pointer)
    used = None       # keys seen while recording
    host = None
    table = None
    count = 0
    blocks = 0
    step = 0
    packed_step = -1  # the step whose begin_step ran the batch launch
    dead = False      # a recorded weight tensor was freed
    retired = []      # workspaces the dropped tables wrote into

    @classmethod
    def invalidate(cls, off=False):
        """drop the descriptor table: nothing launches through its pointers again (outside graphs captured earlier, whose
        buffers stay parked in `retired`)"""
        for k, ent in list(cls.cache.items()):
            if ent[1]:
                cls.retired.append(ent[0])
                del cls.cache[k]
        del cls.retired[:-4 * cls.CAP]
        cls.table, cls.count, cls.blocks, cls.used = None, 0, 0, None
        if cls.state == 'recording':   # stop the library's recorder
            import ctypes
            cnt = (ctypes.c_int * 2)(0, 0)
            lib.fn('dis_convb_pack_record')(None, 0, ctypes.cast(cnt, ctypes.c_void_p))
        cls.state = 'off' if off else 'idle'
        cls.packed_step = -1
        cls.dead = False

    @classmethod
    def _on_dead(cls, key):
        def cb(_ref):
            ent = cls.cache.get(key)
            if ent is None or ent[2] is not _ref:   # (the entry was dropped or re-bound to another tensor since)
                return
            if ent[1] or (cls.used is not None and key in cls.used):
                cls.dead = True     # handled at the next begin_step / workspace call (no library calls from a finalizer)
            else:
                cls.cache.pop(key, None)
        return cb

    @classmethod
    def begin_step(cls, dev):
        cls.step += 1
        if not cls.enabled:
            return
        capturing = torch.cuda.is_current_stream_capturing()
        if cls.dead and not capturing:
            # recorded while the weight was a temporary (died during the record): never batch; died later (its network went away): start over
            cls.invalidate(off=cls.state == 'recording')
        if cls.state == 'recording' and not capturing:
            import ctypes
            cnt = (ctypes.c_int * 2)(0, 0)
            rc = lib.fn('dis_convb_pack_record')(None, 0, ctypes.cast(cnt, ctypes.c_void_p))
            n, cls.blocks = cnt[0], cnt[1]
            if rc == 0 and 0 < n <= cls.CAP:
                nbytes = n * lib.fn('dis_convb_pack_desc_bytes')()
                cls.table = torch.frombuffer(bytearray(cls.host.raw[:nbytes]), dtype=torch.uint8).to(dev)
                cls.count = n
                for k in cls.used:
                    cls.cache[k][1] = True
                cls.state = 'ready'
            else:
                cls.state = 'idle' if n == 0 else 'off'   # (no bf16 convolution ran / more calls than the table holds)
            cls.used = None
        if cls.state == 'ready' and not cls.dead:   # (dead while capturing: the table points at freed weights - no launch, every call packs for itself)
            lib.call('dis_convb_pack_batch', cls.table, cls.count, cls.blocks)
            cls.packed_step = cls.step
            for ent in cls.cache.values():
                if ent[1]:
                    w = ent[2]()
                    ent[3] = w._version if w is not None else -1
        elif cls.state == 'idle' and not capturing:
            import ctypes
            if cls.host is None:
                cls.host = ctypes.create_string_buffer(cls.CAP * lib.fn('dis_convb_pack_desc_bytes')())
            if lib.fn('dis_convb_pack_record')(ctypes.cast(cls.host, ctypes.c_void_p), cls.CAP, None) == 0:
                cls.state, cls.used = 'recording', set()

    @classmethod
    def workspace(cls, key, words, dev, w=None):
        """-> (wpack tensor, prepacked): the call's persistent workspace and whether this step's batch launch has filled it from
        the weight tensor `w` as it is now"""
        if not cls.enabled:
            return torch.empty(words, dtype=torch.int16, device=dev), False
        ent = cls.cache.get(key)
        if ent is not None and (ent[0].numel() != words or ent[0].device != dev):
            if ent[1] or (cls.used is not None and key in cls.used):
                cls.invalidate()        # (the table writes into the old buffer: drop the table, park the buffer)
            cls.cache.pop(key, None)
            ent = None
        if ent is None:
            if len(cls.cache) >= 4 * cls.CAP:
                for k in [k for k, e in cls.cache.items() if not e[1] and not (cls.used is not None and k in cls.used)]:
                    del cls.cache[k]
            import weakref
            ent = cls.cache[key] = [torch.empty(words, dtype=torch.int16, device=dev), False,
                                    weakref.ref(w, cls._on_dead(key)) if w is not None else (lambda: None), -1]
        elif w is not None and ent[2]() is not w:
            # the same address and geometry, another tensor object (a re-created view / a new network at a recycled address)
            if ent[1] or (cls.used is not None and key in cls.used):
                cls.invalidate()
                return cls.workspace(key, words, dev, w)
            import weakref
            ent[2], ent[3] = weakref.ref(w, cls._on_dead(key)), -1
        if cls.state == 'recording' and cls.used is not None:
            cls.used.add(key)
        ok = (ent[1] and cls.state == 'ready' and not cls.dead and cls.packed_step == cls.step and w is not None and
              ent[2]() is w and w._version == ent[3])
        return ent[0], ok


def params_changed():
    """Tell the once-per-step weight packing that parameters were rewritten after this step's batch launch (optimizer step,
    broadcast, checkpoint load): the calls of the rest of this step pack for themselves."""
    _PackBatch.packed_step = -1


def _zeros_d(n, dev):
    a = _ARENA.get(dev)
    if a is not None and a[1] + n <= _ARENA_DOUBLES:
        v = a[0][a[1]:a[1] + n]
        a[1] += (n + 1) // 2 * 2
        a[2] = max(a[2], a[1])
        return v
    return torch.zeros(n, dtype=torch.float64, device=dev)


# --------------------------------------------------------------------------------------------------
# gradient sinks: weight-gradient kernels write straight into the flat gradient buffer of trainer.FlatAdam
# --------------------------------------------------------------------------------------------------
# data_ptr of a parameter -> [view of the flat gradient buffer, written-this-step flag].  The kernels OVERWRITE their
# output, so the first backward use of a parameter in a step may write the view directly and return None to autograd
# (saves one temporary + one `grad += g` launch per parameter, ~236 per DIS-MF step); any further use in the same step
# falls back to returning the gradient for autograd to accumulate.  FlatAdam.zero_grad() re-arms the flags.
_GRAD_SINK = {}
_SINK_NOTIFY = None   # FlatAdam._notify when the bucketed all-reduce is active: told about every finished flat-buffer write
_SINK_PENDING = []    # parameters handed to a kernel by _sink() in the backward that is running


class GradJoin(object):
    """Shared gradient buffer of a tensor that has exactly TWO consumers on the tape (a residual branch, the two heads of
    a fork).  The consumer whose backward runs first stores its input gradient here and returns None to autograd; the
    one that runs second accumulates into the stored buffer inside its own kernel (conv epilogue / atomic scatter /
    row gather) and returns the buffer.  This replaces autograd's separate `g1 + g2` pass over the activation.
    Create one per forward call; tensors may be views of different shape over the same contiguous memory."""

    def __init__(self):
        self.buf = None

    def first(self, g):
        """called by the first producer: keep g, return what autograd should see (nothing)"""
        self.buf = g
        return None

    def take(self, shape):
        b, self.buf = self.buf, None
        return b.view(shape)

    def target(self, like, new=torch.empty_like):
        """-> (buffer the gradient wrt `like` is written into, accumulate): the stored buffer when the other consumer ran first"""
        if self.buf is None:
            return new(like), False
        return self.take(like.shape), True

    def result(self, g, accumulated):
        """what autograd should see once g (from target()) is written"""
        return g if accumulated else self.first(g)


class _SoleConsumer(object):
    """GradJoin's stand-in where the tensor has one consumer: a fresh buffer, the gradient goes to autograd"""

    @staticmethod
    def target(like, new=torch.empty_like):
        return new(like), False

    @staticmethod
    def result(g, accumulated):
        return g


_SOLE = _SoleConsumer()


class GradAccum(object):
    """Shared gradient buffer of a tensor with SEVERAL consumers whose backward kernels accumulate (+= / atomics) into
    their output, e.g. a frame's depth map in the 6 directional flow-consistency terms it takes part in.  Every consumer
    calls use() in its forward; in backward it accumulates into buffer(like) and returns done() to autograd: None for
    all but the consumer that runs last, which hands over the sum.  One zero fill and no autograd adds instead of one
    fill per consumer and a chain of `g1 + g2`.  Create one per tensor and forward pass."""

    def __init__(self):
        self.buf = None
        self.pending = 0

    def use(self):
        self.pending += 1

    def buffer(self, like):
        if self.buf is None:
            self.buf = torch.zeros_like(like)
        return self.buf

    def done(self):
        self.pending -= 1
        if self.pending == 0:
            b, self.buf = self.buf, None
            return b
        return None


def register_grad_sinks(params, notify=None):
    """notify(param): called once the kernel that writes a parameter's gradient straight into the flat buffer has been
    launched (autograd never sees that gradient, so a post-accumulate hook would not fire for it)."""
    global _SINK_NOTIFY
    _GRAD_SINK.clear()
    _SINK_NOTIFY = notify
    del _SINK_PENDING[:]
    for p in params:
        if p.grad is not None:
            _GRAD_SINK[p.data_ptr()] = [p.grad, False]


def reset_grad_sinks():
    for e in _GRAD_SINK.values():
        e[1] = False
    del _SINK_PENDING[:]


def _sinks_written():
    """end of a backward that used _sink(): its kernels are enqueued, the flat-buffer gradients it wrote are final"""
    if _SINK_PENDING:
        if _SINK_NOTIFY is not None:
            for p_ in _SINK_PENDING:
                _SINK_NOTIFY(p_)
        del _SINK_PENDING[:]


def _sink(param):
    """-> (tensor to write the gradient into, value to return to autograd)"""
    e = _GRAD_SINK.get(param.data_ptr())
    # the tensor must really be the registered parameter: its .grad IS the flat view (guards against a stale entry
    # whose address was reused by an unrelated tensor)
    if (e is not None and not e[1] and e[0].shape == param.shape and param.grad is not None
            and param.grad.data_ptr() == e[0].data_ptr()):
        e[1] = True
        _SINK_PENDING.append(param)
        return e[0], None
    g = torch.empty_like(param)
    return g, g


def _unsink(param, got):
    """hand a sink back (the launch it was taken for did not run): the next _sink(param) gets it again"""
    if param is None or got is None or got[1] is not None:
        return
    e = _GRAD_SINK.get(param.data_ptr())
    if e is not None and e[1]:
        e[1] = False
        for i_ in range(len(_SINK_PENDING) - 1, -1, -1):
            if _SINK_PENDING[i_] is param:
                del _SINK_PENDING[i_]
                break


def _sink_opt(param):
    """_sink for an optional parameter (a bias): (None, None) without one.  Parameter gradients leave through the sinks, not
    through autograd's AccumulateGrad nodes: one launch less per parameter, and a captured step (trainer.GraphedStep) then never
    runs an AccumulateGrad node that an earlier, still referenced eager step created on the default stream - joining the
    legacy default stream into a capture crashes the HIP runtime."""
    return _sink(param) if param is not None else (None, None)


def _into_sinks(weight, bias, grads, launch):
    """launch(gw, gb) -> bool writes a weight / bias gradient: into grads = (gw, gb) when given, else into the sinks of weight / bias,
    which go back when the launch did not run (False).  -> (ran, gw_ret, gb_ret)"""
    if grads is not None:
        return launch(*grads), None, None
    got = (_sink(weight), _sink_opt(bias))
    if launch(got[0][0], got[1][0]):
        return True, got[0][1], got[1][1]
    for p_, g_ in zip((weight, bias), got):
        _unsink(p_, g_)
    return False, None, None


def _sink_block(params):
    """Gradient sink for a kernel that writes the gradients of several parameters as ONE contiguous block (Conv3D's
    five arrays): -> flat float view covering all of them if they are registered, unused so far and adjacent in the
    flat gradient buffer in this order, else None (the caller then returns separate tensors to autograd)."""
    es = []
    for p_ in params:
        e = _GRAD_SINK.get(p_.data_ptr())
        if (e is None or e[1] or e[0].shape != p_.shape or p_.grad is None or p_.grad.data_ptr() != e[0].data_ptr()):
            return None
        es.append(e)
    for a, b in zip(es[:-1], es[1:]):
        if b[0].data_ptr() != a[0].data_ptr() + a[0].numel() * 4:
            return None
    for e in es:
        e[1] = True
    _SINK_PENDING.extend(params)
    first = es[0][0]
    return torch.as_strided(first, (sum(e[0].numel() for e in es),), (1,), first.storage_offset())


# --------------------------------------------------------------------------------------------------
# LCN
# --------------------------------------------------------------------------------------------------
def lcn(x, radius=5, eps=0.05):
    """x (N,1,H,W) -> (lcn, std); no gradient (inputs are data).  reference model/networks.py:679-689"""
    x = _c(x)
    _chk(x)
    n, c, h, w = x.shape
    assert c == 1
    out = torch.empty_like(x)
    std = torch.empty_like(x)
    lib.call('dis_lcn_fwd', x, out, std, n, h, w, int(radius), float(eps))
    return out, std


def draw_augment_params(n, rng, max_blur=0.5, max_noise=3.0, max_sp_noise=0.0005):
    """the per-image random choices of the reference's augment_image (data/data_manipulation.py:161-177) with the
    dataset's settings (data/dataset.py:67-70), drawn with a numpy RandomState in the reference's order:
    (n, 6) float32 {blur flag, sigma_im, sigma_amb, noise_im, noise_amb, sp_ratio or -1}"""
    import numpy as np
    out = np.zeros((n, 6), np.float32)
    for i in range(n):
        if rng.uniform(0, 1) < 0.5:
            out[i, 0] = 1.0
            out[i, 1] = rng.uniform(0.2, max_blur)
            out[i, 2] = rng.uniform(0.2, max_blur)
        out[i, 3] = rng.uniform(0.0, max_noise)
        out[i, 4] = rng.uniform(0.0, max_noise)
        out[i, 5] = rng.uniform(0.0, max_sp_noise) if rng.uniform(0, 1) < 0.5 else -1.0
    return out


def augment(im, amb, params, seed):
    """device-side training augmentation (dis_augment): im, amb (..., H, W) float32; params (n,6) float32 and seed (1,) int64
    DEVICE tensors (n = number of H x W planes).  Returns (im_aug, amb_aug); no gradient (inputs are data)."""
    im, amb, params = _c(im), _c(amb), _c(params)
    _chk(im, amb, params)
    h, w = im.shape[-2:]
    n = im.numel() // (h * w)
    if tuple(params.shape) != (n, 6) or seed.dtype != torch.int64 or not seed.is_cuda or amb.shape != im.shape:
        raise RuntimeError('augment: params must be (n,6) float32, seed a CUDA int64 tensor, amb shaped like im')
    ws = torch.empty(2 * n, dtype=torch.int32, device=im.device)
    out_im, out_amb = torch.empty_like(im), torch.empty_like(amb)
    lib.call('dis_augment', im, amb, params, seed, ws, out_im, out_amb, n, h, w)
    return out_im, out_amb


# --------------------------------------------------------------------------------------------------
# photometric
# --------------------------------------------------------------------------------------------------
class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, es, ta, block_size, type, eps):
        es, ta = _c(es), _c(ta)
        _chk(es, ta)
        n, c, h, w = es.shape
        out = torch.empty((n, 1, h, w), dtype=es.dtype, device=es.device)
        lib.call('dis_photometric_fwd', es, ta, out, n, c, h, w, int(block_size), int(type), float(eps))
        ctx.save_for_backward(es, ta)
        ctx.cfg = (int(block_size), int(type), float(eps))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        es, ta = ctx.saved_tensors
        block, type, eps = ctx.cfg
        n, c, h, w = es.shape
        g = _c(grad_out)
        ges = torch.empty_like(es)
        lib.call('dis_photometric_bwd', es, ta, g, ges, n, c, h, w, block, type, eps)
        return ges, None, None, None, None


# DIS_PHOTO_SINGLE_VIA_MULTI=0: a single estimate stays on the general kernels (diagnostics)
PHOTO_SINGLE_VIA_MULTI = _os_env.environ.get('DIS_PHOTO_SINGLE_VIA_MULTI', '1') != '0'


def photometric(es, ta, block_size, type, eps):
    # the census forms at the reference's window (9 x 9, one channel) run the round-4 kernels (csrc/pixel_ops.hip
    # census_*_multi_kernel with one estimate: fused multiply-adds, sign by clamp); everything else the general kernels
    if PHOTO_SINGLE_VIA_MULTI and es.dim() == 4 and photometric_multi_ok(1, es.shape[1], block_size, type):
        return _PhotometricMulti.apply(es.unsqueeze(0), ta, block_size, type, eps)[0]
    return _Photometric.apply(es, ta, block_size, type, eps)


class _PhotometricMulti(torch.autograd.Function):
    """census window loss of S stacked estimates (S, n, 1, h, w) against one target (n, 1, h, w) in one launch
    (dis_photometric_fwd_multi): the target's soft signs are evaluated once for all S."""

    @staticmethod
    def forward(ctx, es, ta, block_size, type, eps):
        es, ta = _c(es), _c(ta)
        _chk(es, ta)
        s, n, c, h, w = es.shape
        assert c == 1 and tuple(ta.shape) == (n, 1, h, w)
        out = torch.empty_like(es)
        lib.call('dis_photometric_fwd_multi', es, ta, out, s, n, h, w, int(block_size), int(type), float(eps))
        ctx.save_for_backward(es, ta)
        ctx.cfg = (int(block_size), int(type), float(eps))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        es, ta = ctx.saved_tensors
        block, type, eps = ctx.cfg
        s, n, _, h, w = es.shape
        ges = torch.empty_like(es)
        lib.call('dis_photometric_bwd_multi', es, ta, _c(grad_out), ges, s, n, h, w, block, type, eps)
        return ges, None, None, None, None


# DIS_PHOTO_LOSS_ONE_NODE=0: pattern warp, census loss and weighted mean of the S estimates as separate autograd nodes (A/B)
PHOTO_LOSS_ONE_NODE = _os_env.environ.get('DIS_PHOTO_LOSS_ONE_NODE', '1') != '0'


def photometric_multi_ok(n_estimates, channels, block_size, type):
    return 1 <= n_estimates <= 4 and channels == 1 and int(block_size) == 9 and int(type) in (2, 3)


def photometric_multi(es_list, ta, block_size, type, eps):
    """[photometric(es, ta, ...) for es in es_list] in one launch (census types, 9 x 9, one channel, <= 4 estimates)."""
    out = _PhotometricMulti.apply(torch.stack([_c(e) for e in es_list], 0), ta, block_size, type, eps)
    return list(out.unbind(0))


# --------------------------------------------------------------------------------------------------
# pattern projection
# --------------------------------------------------------------------------------------------------
class _PatternWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, disp):
        pattern, disp = _c(pattern), _c(disp)
        _chk(pattern, disp)
        n, _, h, w = disp.shape
        assert pattern.numel() == h * w
        proj = torch.empty_like(disp)
        lib.call('dis_pattern_warp_fwd', pattern, disp, proj, n, h, w)
        ctx.save_for_backward(pattern, disp)
        return proj

    @staticmethod
    def backward(ctx, g):
        pattern, disp = ctx.saved_tensors
        n, _, h, w = disp.shape
        gd = torch.empty_like(disp)
        lib.call('dis_pattern_warp_bwd', pattern, disp, _c(g), gd, n, h, w)
        return None, gd


def pattern_warp(pattern, disp):
    return _PatternWarp.apply(pattern, disp)


class _PatternPhotoLossMulti(torch.autograd.Function):
    """[weighted_mean(photometric(pattern_warp(pattern, d), ta), std) for d in disps] as ONE autograd node: the S projections are
    written into the slices of one (S, n, 1, h, w) buffer, the census loss of all S runs in one launch (dis_photometric_fwd_multi)
    and the S weighted means read its slices - and on the way back the S mean gradients are written into the slices of ONE buffer.
    As separate nodes (pattern_warp, photometric_multi over torch.stack, weighted_mean over unbind) autograd moved the S maps
    through a stack on the way in and a cat on the way back: 2 x 113 MB of copies per DIS-SF bs = 8 step.  Same launches, same
    arithmetic per launch as the separate nodes (reference model/single_frame_worker.py:110-118 -> model/networks.py:336-377)."""

    @staticmethod
    def forward(ctx, pattern, ta, std, block_size, type, eps, *disps):
        pattern, ta = _c(pattern), _c(ta)
        std = _c(std) if std is not None else None
        disps = [_c(d) for d in disps]
        _chk(pattern, ta, std, *disps)
        s = len(disps)
        n, c, h, w = disps[0].shape
        assert c == 1 and tuple(ta.shape) == (n, 1, h, w) and pattern.numel() == h * w
        assert all(tuple(d.shape) == (n, 1, h, w) for d in disps)
        proj = torch.empty((s, n, 1, h, w), dtype=torch.float32, device=ta.device)
        for k in range(s):
            lib.call('dis_pattern_warp_fwd', pattern, disps[k], proj[k], n, h, w)
        diff = torch.empty_like(proj)
        lib.call('dis_photometric_fwd_multi', proj, ta, diff, s, n, h, w, int(block_size), int(type), float(eps))
        accs = _zeros_d(2 * s, ta.device)
        outs = torch.empty(s, dtype=torch.float32, device=ta.device)
        for k in range(s):
            lib.call('dis_weighted_mean_fwd', diff[k], std, accs[2 * k:2 * k + 2], outs[k:k + 1], diff[k].numel())
        ctx.save_for_backward(pattern, ta, std, proj, accs, *disps)
        ctx.cfg = (int(block_size), int(type), float(eps), s)
        return tuple(outs[k] for k in range(s))

    @staticmethod
    def backward(ctx, *gs):
        pattern, ta, std, proj, accs = ctx.saved_tensors[:5]
        disps = ctx.saved_tensors[5:]
        block, type, eps, s = ctx.cfg
        n, _, h, w = disps[0].shape
        gdiff = torch.empty_like(proj)
        for k in range(s):
            g = gs[k] if gs[k] is not None else torch.zeros((), dtype=torch.float32, device=proj.device)
            lib.call('dis_weighted_mean_bwd', std, accs[2 * k:2 * k + 2], _c(g), gdiff[k], gdiff[k].numel())
        gproj = torch.empty_like(proj)
        lib.call('dis_photometric_bwd_multi', proj, ta, gdiff, gproj, s, n, h, w, block, type, eps)
        gds = []
        for k in range(s):
            gd = torch.empty_like(disps[k])
            lib.call('dis_pattern_warp_bwd', pattern, disps[k], gproj[k], gd, n, h, w)
            gds.append(gd)
        return (None, None, None, None, None, None) + tuple(gds)


def pattern_photo_loss_multi(pattern, disps, ta, std, block_size, type, eps):
    """per-estimate census loss values (device scalars) of the pattern warped by each disparity map against one image"""
    return list(_PatternPhotoLossMulti.apply(pattern, ta, std, block_size, type, eps, *disps))


# --------------------------------------------------------------------------------------------------
# scalar reductions
# --------------------------------------------------------------------------------------------------
class _WeightedMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x = _c(x)
        w = _c(w) if w is not None else None
        _chk(x, w)
        acc = _zeros_d(2, x.device)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        lib.call('dis_weighted_mean_fwd', x, w, acc, out, x.numel())
        ctx.save_for_backward(w, acc) if w is not None else ctx.save_for_backward(acc)
        ctx.has_w = w is not None
        ctx.shape = x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.has_w:
            w, acc = ctx.saved_tensors
        else:
            (acc,) = ctx.saved_tensors
            w = None
        gx = torch.empty(ctx.shape, dtype=torch.float32, device=acc.device)
        lib.call('dis_weighted_mean_bwd', w, acc, _c(g), gx, gx.numel())
        return gx, None


def weighted_mean(x, w=None):
    """sum(w*x)/sum(w)  (w None => mean)"""
    return _WeightedMean.apply(x, w)


class LossTerms(list):
    """The weighted loss terms a worker's loss_forward returns (a list of device scalars, as the reference returns them) that also
    carries `total`, their sum as ONE autograd node, and `weighted`, the same values as one vector."""
    total = None
    weighted = None


_WVEC = {}


class _WeightedTotal(torch.autograd.Function):
    """total = sum_i w_i * val_i over a worker's loss terms in three launches (stack, multiply, sum) and one on the way back, instead
    of two elementwise launches per term each way plus a chain of scalar additions (reference model/multi_frame_worker.py:103-175,
    single_frame_worker.py:101-165: `val * 0.2 / ge_num`, `sum(errs)`): ~45 launches of 5 us per DIS-MF step."""

    @staticmethod
    def forward(ctx, wvec, *vals):
        weighted = torch.stack([v.reshape(()) for v in vals]) * wvec
        ctx.save_for_backward(wvec)
        ctx.set_materialize_grads(False)
        return weighted.sum(), weighted

    @staticmethod
    def backward(ctx, gtotal, gw):
        # (gtotal: through `total`, the step's path; gw: through the individual terms, for a caller that sums them itself)
        wvec, = ctx.saved_tensors
        g = wvec * gtotal if gtotal is not None else None
        if gw is not None:
            g = wvec * gw if g is None else g + wvec * gw
        return (None,) + tuple(g.unbind(0))


def weighted_terms(pairs):
    """pairs: [(unweighted loss value: device scalar, weight: python float)] -> LossTerms of the weighted values"""
    ws = tuple(float(w) for _, w in pairs)
    dev = pairs[0][0].device
    wvec = _WVEC.get((ws, dev))
    if wvec is None:   # (created by the first, eager step; a captured step finds it)
        wvec = _WVEC[(ws, dev)] = torch.tensor(ws, dtype=torch.float32, device=dev)
    total, weighted = _WeightedTotal.apply(wvec, *[v for v, _ in pairs])
    out = LossTerms(weighted.unbind(0))
    out.total, out.weighted = total, weighted
    return out


class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        _chk(a, b)
        acc = _zeros_d(1, a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        lib.call('dis_l1_mean_fwd', a, b, acc, out, a.numel())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a)
        lib.call('dis_l1_mean_bwd', a, b, _c(g), ga, a.numel())
        return ga, None


def l1_mean(a, b):
    return _L1Mean.apply(a, b)


class _SgmL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o, sgm, noise, thresh):
        o, sgm, noise = _c(o), _c(sgm), _c(noise)
        _chk(o, sgm, noise)
        acc = _zeros_d(2, o.device)
        out = torch.empty((), dtype=torch.float32, device=o.device)
        lib.call('dis_sgm_l1_fwd', o, sgm, noise, float(thresh), acc, out, o.numel())
        ctx.save_for_backward(o, sgm, noise, acc)
        ctx.thresh = float(thresh)
        return out

    @staticmethod
    def backward(ctx, g):
        o, sgm, noise, acc = ctx.saved_tensors
        go = torch.empty_like(o)
        lib.call('dis_sgm_l1_bwd', o, sgm, noise, ctx.thresh, acc, _c(g), go, o.numel())
        return go, None, None, None


def sgm_l1(o, sgm_disp, noise, thresh=30.0):
    """sum(|o - sgm + noise| * (sgm > thresh)) / sum(sgm > thresh)  (the `real`-data warm-up term)"""
    return _SgmL1.apply(o, sgm_disp, noise, thresh)


def _ptr_table(tensors):
    """a host array of the tensors' device addresses (the entry point copies them into its kernel arguments)"""
    return (_ct.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _MaskedL1Multi(torch.autograd.Function):
    """[masked mean |o - target| for o in outs] as ONE autograd node: one accumulate and one finalize launch forward, one launch
    backward (dis_masked_l1_multi_fwd / _bwd), whatever the number of estimates.  A pixel counts when target > 0 over its whole
    (2 erode + 1)^2 window; the count is shared by the estimates and stays on the device (no valid pixel: values and gradients 0)."""

    @staticmethod
    def forward(ctx, target, erode, *outs):
        target = _c(target)
        outs = [_c(o) for o in outs]
        _chk(target, *outs)
        n = len(outs)
        if not 1 <= n <= 4:
            raise RuntimeError(f'masked_l1_multi: 1 .. 4 estimates, not {n}')
        if int(erode) != erode or not 0 <= erode <= 3:
            raise RuntimeError(f'masked_l1_multi: erode is an integer in 0 .. 3, not {erode!r}')
        shape = tuple(target.shape)
        if len(shape) not in (4, 5) or shape[-3] != 1:
            raise RuntimeError(f'masked_l1_multi: target of shape {shape}: (tl, bs, 1, H, W) or (N, 1, H, W) is expected')
        if any(tuple(o.shape) != shape for o in outs):
            raise RuntimeError(f'masked_l1_multi: estimates of shapes {[tuple(o.shape) for o in outs]} against a target of {shape}')
        h, w = shape[-2:]
        planes = target.numel() // (h * w) if h * w else 0
        acc = torch.empty(lib.fn('dis_masked_l1_multi_acc_doubles')(), dtype=torch.float64, device=target.device)
        vals = torch.empty(n, dtype=torch.float32, device=target.device)
        lib.call('dis_masked_l1_multi_fwd', _ptr_table(outs), n, target, int(erode), acc, vals, planes, h, w)
        ctx.save_for_backward(target, acc, *outs)
        ctx.cfg = (int(erode), planes, h, w)
        return tuple(vals[k] for k in range(n))

    @staticmethod
    def backward(ctx, *gs):
        target, acc = ctx.saved_tensors[:2]
        outs = ctx.saved_tensors[2:]
        erode, planes, h, w = ctx.cfg
        zero = None
        if any(g is None for g in gs):
            zero = torch.zeros((), dtype=torch.float32, device=target.device)
        gscale = torch.stack([g.reshape(()).float() if g is not None else zero for g in gs])
        grads = [torch.empty_like(o) for o in outs]
        lib.call('dis_masked_l1_multi_bwd', _ptr_table(outs), len(outs), target, erode, acc, gscale, _ptr_table(grads), planes, h, w)
        return (None, None) + tuple(grads)


def masked_l1_multi(outs, target, erode=0):
    """per-estimate sum(|o - target| over valid) / count(valid) (a list of device scalars), valid = target > 0 over the whole
    (2 erode + 1)^2 window inside the image: the pseudo-GT term on a target with holes (<track>/raycast_<disp>.npz)"""
    return list(_MaskedL1Multi.apply(target, erode, *outs))


class _SmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, amb):
        disp, amb = _c(disp), _c(amb)
        _chk(disp, amb)
        n, _, h, w = disp.shape
        acc = _zeros_d(1, disp.device)
        out = torch.empty((), dtype=torch.float32, device=disp.device)
        lib.call('dis_smooth_loss_fwd', disp, amb, acc, out, n, h, w)
        ctx.save_for_backward(disp, amb)
        return out

    @staticmethod
    def backward(ctx, g):
        disp, amb = ctx.saved_tensors
        n, _, h, w = disp.shape
        gd = torch.empty_like(disp)
        ws = torch.empty((n, 2, h, w), dtype=torch.float32, device=disp.device)
        lib.call('dis_smooth_loss_bwd', disp, amb, _c(g), gd, ws, n, h, w)
        return gd, None


def smooth_loss(disp, amb):
    return _SmoothLoss.apply(disp, amb)


class _DispToDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, bf):
        disp = _c(disp)
        _chk(disp)
        depth = torch.empty_like(disp)
        lib.call('dis_disp_to_depth_fwd', disp, depth, float(bf), disp.numel())
        ctx.save_for_backward(disp)
        ctx.bf = float(bf)
        return depth

    @staticmethod
    def backward(ctx, g):
        (disp,) = ctx.saved_tensors
        gd = torch.empty_like(disp)
        lib.call('dis_disp_to_depth_bwd', disp, _c(g), gd, ctx.bf, disp.numel())
        return gd, None


def disp_to_depth(disp, bf):
    return _DispToDepth.apply(disp, bf)


# DIS_GEO_BWD=det: the backward of the flow-consistency loss through dis_geo_loss_bwd_det / _bwd_multi_det - integer sums per term,
# one fp32 rounding per pixel, bit for bit the same on every call.  'atomic' (default): float atomics, equal to rounding.
GEO_BWD_DET = {'atomic': False, 'det': True}[_os_env.environ.get('DIS_GEO_BWD', 'atomic')]


def set_geo_bwd_det(on):
    """select the order-free (True) or the atomic (False) backward of the flow-consistency loss; -> the previous setting"""
    global GEO_BWD_DET
    prev, GEO_BWD_DET = GEO_BWD_DET, bool(on)
    return prev


def _geo_det_workspace(nterms, bs, h, w, device):
    return torch.empty(lib.fn('dis_geo_loss_bwd_det_workspace')(nterms, bs, h, w), dtype=torch.uint8, device=device)


class _GeoLossDir(torch.autograd.Function):
    """One direction of the flow-consistency loss (dis_geo_loss_fwd/bwd)."""

    @staticmethod
    def forward(ctx, depth0, depth1, flow0, flow1, amb0, amb1, pdepth1, R0, t0, R1, t1, K, Kinv, clamp, accs):
        ctx.accs = accs  # optional (GradAccum of depth0, GradAccum of depth1)
        if accs is not None:
            accs[0].use()
            accs[1].use()
        ts = [_c(t) for t in (depth0, depth1, flow0, flow1, amb0, amb1)]
        depth0, depth1, flow0, flow1, amb0, amb1 = ts
        pdepth1 = _c(pdepth1) if pdepth1 is not None else None
        R0, t0, R1, t1 = _c(R0), _c(t0), _c(R1), _c(t1)
        _chk(depth0, depth1, flow0, flow1, amb0, amb1, pdepth1, R0, t0, R1, t1)
        bs, _, h, w = depth0.shape
        mask = torch.empty_like(depth0)
        acc = torch.empty(lib.fn('dis_geo_loss_acc_doubles')(), dtype=torch.float64, device=depth0.device)  # sums + block slots
        out = torch.empty((), dtype=torch.float32, device=depth0.device)
        lib.call('dis_geo_loss_fwd', depth0, depth1, flow0, flow1, amb0, amb1, pdepth1, R0, t0, R1, t1, K, Kinv,
                 float(clamp), mask, acc, out, bs, h, w)
        ctx.save_for_backward(depth0, depth1, flow0, R0, t0, R1, t1, mask, acc)
        ctx.cfg = (K, Kinv, float(clamp))
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)  # no zero tensor for the mask's (non-existent) gradient
        return out, mask

    @staticmethod
    def backward(ctx, g, _gmask):
        depth0, depth1, flow0, R0, t0, R1, t1, mask, acc = ctx.saved_tensors
        K, Kinv, clamp = ctx.cfg
        bs, _, h, w = depth0.shape
        accs = ctx.accs
        g0 = accs[0].buffer(depth0) if accs is not None else torch.zeros_like(depth0)
        g1 = accs[1].buffer(depth1) if accs is not None else torch.zeros_like(depth1)
        if GEO_BWD_DET:   # order-free sums: the same bits on every call (g0, g1 are added to, as below)
            lib.call('dis_geo_loss_bwd_det', depth0, depth1, flow0, R0, t0, R1, t1, K, Kinv, clamp, mask, acc, _c(g), g0, g1,
                     bs, h, w, _geo_det_workspace(1, bs, h, w, depth0.device))
        else:
            lib.call('dis_geo_loss_bwd', depth0, depth1, flow0, R0, t0, R1, t1, K, Kinv, clamp, mask, acc, _c(g), g0, g1,
                     bs, h, w)  # accumulates into g0 (+=) and g1 (atomics)
        if accs is not None:
            g0, g1 = accs[0].done(), accs[1].done()
        return (g0, g1) + (None,) * 13


def geo_loss_dir(depth0, depth1, flow0, flow1, amb0, amb1, pdepth1, R0, t0, R1, t1, K, Kinv, clamp=-1.0, accs=None):
    """K, Kinv: lib.host_floats(9).  accs: optional (GradAccum, GradAccum) shared gradient buffers of depth0 / depth1.
    Returns (loss, mask)."""
    return _GeoLossDir.apply(depth0, depth1, flow0, flow1, amb0, amb1, pdepth1, R0, t0, R1, t1, K, Kinv, clamp, accs)


import ctypes as _ct
import os as _os
GEO_MULTI = _os.environ.get('DIS_GEO_MULTI', '1') != '0'   # =0: one launch per directional term (dis_geo_loss_fwd / _bwd)
GEO_MULTI_MAX = 16


class _GeoTerm(_ct.Structure):   # include/dis_hip.h: DisGeoTerm
    _fields_ = [(n_, _ct.c_void_p) for n_ in ('depth0', 'depth1', 'flow0', 'flow1', 'amb0', 'amb1', 'pdepth1', 'R0', 't0', 'R1', 't1',
                                              'mask', 'gdepth0', 'gdepth1')]


class _GeoLossAll(torch.autograd.Function):
    """Every directional flow-consistency term of a step in one forward and one backward launch (dis_geo_loss_fwd_multi / _bwd_multi).
    depth / amb / pdepth (tl, bs, 1, h, w), R (tl, bs, 3, 3), t (tl, bs, 3); pairs: ((i0, i1), ...) one per term; flows: per term
    flow_{i0 i1}, flow_{i1 i0}.  Returns the (len(pairs),) vector of term values."""

    @staticmethod
    def _table(pairs, depth, R, t, mask, flows0, flows1=None, amb=None, pdepth=None, gdepth=None):
        tl, bs = depth.shape[0], depth.shape[1]
        fs = depth[0].numel() * 4
        tab = (_GeoTerm * len(pairs))()
        for k, (i0, i1) in enumerate(pairs):
            q = tab[k]
            q.depth0, q.depth1 = depth.data_ptr() + i0 * fs, depth.data_ptr() + i1 * fs
            q.flow0 = flows0[k].data_ptr()
            q.R0, q.R1 = R.data_ptr() + i0 * bs * 36, R.data_ptr() + i1 * bs * 36
            q.t0, q.t1 = t.data_ptr() + i0 * bs * 12, t.data_ptr() + i1 * bs * 12
            q.mask = mask.data_ptr() + k * fs
            if flows1 is not None:
                q.flow1 = flows1[k].data_ptr()
                q.amb0, q.amb1 = amb.data_ptr() + i0 * fs, amb.data_ptr() + i1 * fs
                q.pdepth1 = pdepth.data_ptr() + i1 * fs if pdepth is not None else None
            if gdepth is not None:
                q.gdepth0, q.gdepth1 = gdepth.data_ptr() + i0 * fs, gdepth.data_ptr() + i1 * fs
        return tab

    @staticmethod
    def forward(ctx, depth, amb, pdepth, R, t, K, Kinv, clamp, pairs, *flows):
        depth, amb, R, t = _c(depth), _c(amb), _c(R), _c(t)
        pdepth = _c(pdepth) if pdepth is not None else None
        flows = [_c(f) for f in flows]
        _chk(depth, amb, pdepth, R, t, *flows)
        tl, bs, _, h, w = depth.shape
        T = len(pairs)
        assert len(flows) == 2 * T and T <= GEO_MULTI_MAX and amb.shape == depth.shape and (pdepth is None or pdepth.shape == depth.shape)
        assert tuple(R.shape) == (tl, bs, 3, 3) and tuple(t.shape) == (tl, bs, 3) and all(tuple(f.shape) == (bs, 2, h, w) for f in flows)
        mask = torch.empty((T, bs, 1, h, w), dtype=torch.float32, device=depth.device)
        acc = torch.empty(lib.fn('dis_geo_loss_multi_acc_doubles')(T), dtype=torch.float64, device=depth.device)
        out = torch.empty(T, dtype=torch.float32, device=depth.device)
        tab = _GeoLossAll._table(pairs, depth, R, t, mask, flows[0::2], flows[1::2], amb, pdepth)
        lib.call('dis_geo_loss_fwd_multi', tab, T, K, Kinv, float(clamp), acc, out, bs, h, w)
        ctx.save_for_backward(depth, R, t, mask, acc, *flows[0::2])
        ctx.cfg = (K, Kinv, float(clamp), pairs)
        return out

    @staticmethod
    def backward(ctx, g):
        depth, R, t, mask, acc = ctx.saved_tensors[:5]
        flows0 = ctx.saved_tensors[5:]
        K, Kinv, clamp, pairs = ctx.cfg
        tl, bs, _, h, w = depth.shape
        gd = torch.zeros_like(depth)
        tab = _GeoLossAll._table(pairs, depth, R, t, mask, flows0, gdepth=gd)
        if GEO_BWD_DET:
            lib.call('dis_geo_loss_bwd_multi_det', tab, len(pairs), K, Kinv, clamp, acc, _c(g.float()), bs, h, w,
                     _geo_det_workspace(len(pairs), bs, h, w, depth.device))
        else:
            lib.call('dis_geo_loss_bwd_multi', tab, len(pairs), K, Kinv, clamp, acc, _c(g.float()), bs, h, w)
        return (gd,) + (None,) * (8 + 2 * len(pairs))


def geo_loss_all(depth, amb, pdepth, R, t, K, Kinv, clamp, pairs, flows):
    """all directional terms at once: pairs ((i0, i1), ...), flows [(flow_{i0 i1}, flow_{i1 i0}), ...] -> (len(pairs),) values"""
    flat = [f for pr in flows for f in pr]
    return _GeoLossAll.apply(depth, amb, pdepth, R, t, K, Kinv, clamp, tuple(pairs), *flat)


# --------------------------------------------------------------------------------------------------
# layout helpers (no gradient: they only touch network inputs)
# --------------------------------------------------------------------------------------------------
def pack4_nhwc(srcs, n, h, w):
    """srcs: list of up to 4 (tensor, sample_stride_in_floats) or None -> (n,h,w,4) nhwc."""
    dev = next(s[0] for s in srcs if s is not None).device
    out = torch.empty((n, h, w, 4), dtype=torch.float32, device=dev)
    args = []
    for i in range(4):
        s = srcs[i] if i < len(srcs) else None
        if s is None:
            args += [None, 0]
        else:
            args += [s[0], int(s[1])]
    lib.call('dis_pack4_nhwc_strided', *args, out, n, h, w)
    return out


def planar_to_nhwc(x):
    x = _c(x)
    _chk(x)
    n, c, h, w = x.shape
    y = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    lib.call('dis_planar_to_nhwc', x, y, n, c, h, w)
    return y


def nhwc_to_planar(x):
    x = _c(x)
    _chk(x)
    n, h, w, c = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    lib.call('dis_nhwc_to_planar', x, y, n, c, h, w)
    return y


class _ResizePlanar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, align_corners, scale0, scale1, c_for_scale):
        x = _c(x)
        _chk(x)
        lead = x.shape[:-2]
        hin, win = x.shape[-2:]
        nc = 1
        for d in lead:
            nc *= d
        y = torch.empty((*lead, size[0], size[1]), dtype=torch.float32, device=x.device)
        lib.call('dis_resize_bilinear_planar_fwd', x, y, nc, hin, win, size[0], size[1], int(align_corners),
                 float(scale0), float(scale1), int(c_for_scale))
        ctx.cfg = (nc, hin, win, size[0], size[1], int(align_corners), x.shape, int(c_for_scale))
        return y

    @staticmethod
    def backward(ctx, g):
        nc, hin, win, ho, wo, ac, shape, cfs = ctx.cfg
        if cfs != 0:
            raise RuntimeError('resize with flow scaling has no backward (flows are data)')
        gx = torch.empty(shape, dtype=torch.float32, device=g.device)
        lib.call('dis_resize_bilinear_planar_bwd', _c(g), gx, nc, hin, win, ho, wo, ac)
        return gx, None, None, None, None, None


def resize_planar(x, size, align_corners=True, flow_scale=None):
    """bilinear resize over the last two dims of a planar tensor.  flow_scale=(sx,sy) multiplies channel 0/1
    of a (...,2,H,W) flow tensor (reference resize_flow_like)."""
    if flow_scale is None:
        return _ResizePlanar.apply(x, tuple(size), align_corners, 1.0, 1.0, 0)
    assert x.shape[-3] == 2
    return _ResizePlanar.apply(x, tuple(size), align_corners, flow_scale[0], flow_scale[1], 2)


class _ResizeNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, align_corners):
        x = _c(x)
        _chk(x)
        n, hin, win, c = x.shape
        y = torch.empty((n, size[0], size[1], c), dtype=torch.float32, device=x.device)
        lib.call('dis_resize_bilinear_nhwc_fwd', x, y, n, hin, win, size[0], size[1], c, int(align_corners))
        ctx.cfg = (n, hin, win, size[0], size[1], c, int(align_corners))
        return y

    @staticmethod
    def backward(ctx, g):
        n, hin, win, ho, wo, c, ac = ctx.cfg
        gx = torch.empty((n, hin, win, c), dtype=torch.float32, device=g.device)
        lib.call('dis_resize_bilinear_nhwc_bwd', _c(g), gx, n, hin, win, ho, wo, c, ac)
        return gx, None, None


def resize_nhwc(x, size, align_corners=True):
    return _ResizeNHWC.apply(x, tuple(size), align_corners)


# --------------------------------------------------------------------------------------------------
# convolution (MFMA implicit GEMM)
# --------------------------------------------------------------------------------------------------
def _pack_w(weight, cin_pad, mode):
    cout, cin, k, _ = weight.shape
    packed = torch.empty(k * k * cin_pad * cout, dtype=torch.float32, device=weight.device)
    lib.call('dis_conv2d_pack_weights', weight, packed, cout, cin, cin_pad, k, mode)
    return packed


import os as _os
BF16X3 = _os.environ.get('DIS_CONV_BF16X3', '1') != '0'


K4S2_F2 = _os.environ.get('DIS_K4S2_F2', '1') != '0'   # DIS_K4S2_F2=0: the 4 x 4 stride-2 forward on the exact-fp32 MFMA kernel


def _dgrad_k4s2(gpre, weight, gx, n, hin, win, cin, cout, accumulate):
    """input gradient of a 4 x 4 stride-2 pad-1 conv: the one-launch two-term kernel for 32 -> 32 (csrc/conv_k4s2.hip), else - other
    channel counts, the three-term mode, DIS_K4S2_F2=0 - the four parity launches on the exact-fp32 kernel"""
    if (BF16X3 and K4S2_F2 and cin == 32 and cout == 32 and weight.is_contiguous() and
            lib.call_try('dis_conv2d_dgrad_k4s2_f16x2', gpre, weight, gx, n, hin, win, 1 if accumulate else 0)):
        return
    ws = torch.empty(16 * cin * cout, dtype=torch.float32, device=gx.device)
    lib.call('dis_conv2d_dgrad_strided', gpre, weight, gx, ws, n, hin, win, cin, cout, 4, 2, 1, 1 if accumulate else 0)


def _conv_wgrad_any(x, gpre, gw, gb, ws, n, hin, win, cin_pad, cin, cout, k, stride, pad):
    """dis_conv2d_wgrad, or its bf16x3 form for 3x3 stride-1 layers with 16 / 32 channels on both sides."""
    name = 'dis_conv2d_wgrad'
    if BF16X3 and cin_pad in (16, 32) and cout in (16, 32) and k == 3 and stride == 1:
        name = 'dis_conv2d_wgrad_bf16x3'
    lib.call(name, x, gpre, gw, gb, ws, n, hin, win, cin_pad, cin, cout, k, stride, pad)


def _conv_fwd_any(x, weight, cin_pad, mode, bias, y, stats, n, hin, win, cin, cout, k, stride, pad, act):
    """dis_conv2d_fwd, or its bf16x3 form (fp32 accuracy on the bf16 matrix cores) for 3x3 stride-1 layers with 16 / 32
    channels on both sides.  `weight` is the module's OIHW tensor, `mode` the weight order (0 forward, 1 stride-1 input
    gradient); `cin` / `cout` are the channel counts of x and y in THIS call (swapped for the input gradient)."""
    if (BF16X3 and K4S2_F2 and (cin, cout, k, stride, pad) == (32, 32, 4, 2, 1) and weight.is_contiguous() and
            lib.call_try('dis_conv2d_fwd_k4s2_f16x2', x, weight, bias, y, stats, n, hin, win, act)):
        return   # (FuseNet's 4 x 4 stride-2 down convolution on the two-term kernel; under the three-term mode the call says unsupported)
    if BF16X3 and cin in (16, 32) and cout in (16, 32) and k == 3 and stride == 1:
        # `weight` may be a slice w[:, a:b] of a wider weight (conv2d_multi): the kernel reads it through its row stride
        assert weight.stride(1) == 9 and weight.stride(2) == 3 and weight.stride(3) == 1
        lib.call('dis_conv2d_fwd_bf16x3_oihw', x, weight, mode, weight.shape[0], weight.shape[1], weight.stride(0), bias, y,
                 stats, n, hin, win, cin, cout, k, stride, pad, act)
    else:
        lib.call('dis_conv2d_fwd', x, _pack_w(_c(weight), cin_pad, mode), bias, y, stats, n, hin, win, cin, cout, k, stride,
                 pad, act)


# Round 6: input gradient + weight gradient of a 3x3 stride-1 conv 32 -> 32 in ONE launch (dis_conv2d_bwd_fused_f16x2,
# csrc/conv_bwd_fused.hip): the gy halo a tile stages feeds both products, gpre (the GroupNorm-backward pass formed on load) is never
# written, x and gy are read once.  Same-box: 0.79 - 0.95 of the two launches per layer, DIS-MF step 513.9 -> 537.6 frames/s
# (profiles/r6_bwd_fused.md).  DIS_BWD_FUSED=0 keeps the two launches.
BWD_FUSED = _os.environ.get('DIS_BWD_FUSED', '1') != '0'
_FUSED_WS = {}
# The forms the three-term split sends to the one-launch backward (dis_conv2d_bwd_fused_bf16x3): plain, plain_accum, act, act_accum,
# xgn.  At the DIS-MF step's layer shapes every form measured 1 - 5 % SLOWER fused than as its two launches
# (scripts/bwd_fused_strict_forms.py), so none is on by default; DIS_BWD_FUSED_STRICT=all (or a comma list of
# forms) selects them.
BWD_FUSED_STRICT_FORMS = ('plain', 'plain_accum', 'act', 'act_accum', 'xgn')
_strict_env = _os.environ.get('DIS_BWD_FUSED_STRICT', '')
BWD_FUSED_STRICT = frozenset(BWD_FUSED_STRICT_FORMS if _strict_env == 'all' else [f for f in _strict_env.split(',') if f])
_FUSED3_WS = {}


def _with_stats(ctx, y, stats):
    """a conv forward's outputs (y, stats | None); the statistics have no gradient (and get no zero tensor for one)"""
    if stats is not None:
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
    return y, stats


def _bx_shape(cin, cout, k, stride):
    return BF16X3 and cin in (16, 32) and cout in (16, 32) and k == 3 and stride == 1


def _conv_bwd_slice(weight, x, gx, accumulate, grads=None, bias=None, pad=1, lz=None, gy=None, act=ACT_NONE, y=None, xgn=None,
                    sums=None, keep_gpre=False, after_dgrad=None):
    """Both gradients of one stride-1 conv weight slice: a conv2d, a conv2d_gn_in, one source of conv2d_multi.  Which launches
    serve which form is decided here and nowhere else.
      operand: lz, a GroupNorm token (_gn_lazy_pop), whose elementwise pass the input-gradient launch forms on load; else gy, taken
               times act'(y) on load when act != ACT_NONE (the bf16x3 shapes) and as the pre-activation gradient otherwise
      x: the conv's input; xgn = (stats, gamma, beta, eps): the conv stages GroupNorm(x) (conv2d_gn_in)
      gx: input-gradient target (None: not wanted), accumulate: add to what it holds; sums = (ab_x, ab_act): its launch also leaves
          the GroupNorm-backward channel sums of ab_x - without xgn for the GroupNorm that produced x (_GN_PRE).  With an activation
          operand (16 <-> 32, ab_act is x, not accumulating) gx is WRITTEN times act'(x): final_conv, ref_conv's 16-channel source
      grads = (gw, gb): the weight / bias gradient targets (gw may be a slice of a wider gradient); None: the sinks of weight / bias
      keep_gpre: the operand formed from a token is stored for the caller (conv2d_multi's other sources read it)
      after_dgrad(ab, slots): runs once the input gradient is written, before the weight gradient (the GroupNorm backward of xgn)
    -> (the weight gradient's operand, gw_ret, gb_ret, what after_dgrad returned)"""
    cout, cin, k, _ = weight.shape
    n, h, w, cin_pad = x.shape
    split = lib.fn('dis_get_conv_split')() == 1
    epi = gx is not None and sums is not None and split and act == ACT_NONE and cin == cout and _bx_shape(cin, cout, k, 1)
    # the same sums behind an activation operand (dis_conv2d_dgrad_bf16x3_act_gnsums_res's form)
    epi_act = (gx is not None and sums is not None and split and act == ACT_SELU and lz is None and xgn is None and not accumulate and
               (cin, cout) in ((16, 32), (32, 16)) and sums[1] is x and cin_pad == cin and (k, pad) == (3, 1) and _bx_shape(cin, cout, k, 1))
    if lz is not None and not (gx is not None and split and act == ACT_NONE and cin_pad == cin and
                               _gn_lazy_shape(cin, cout, k, 1, pad) and (xgn is None or epi)):
        gy, lz = _gn_lazy_materialize(lz), None
    # one launch for both gradients (csrc/conv_bwd_fused.hip, 32 -> 32): it forms a token's operand (and stores it only in the
    # GroupNorm-on-load form) or takes gy (no epilogue then)
    # (csrc/conv_bwd_fused_c16.hip: the layers with 16 channels on a side, through an entry point of their own - its workspace
    #  function answers -1 for a pair of channel counts without a kernel; a padded input keeps the two launches.  At 16 -> 16 only a
    #  token's forms go there: a plain gy keeps the stand-alone weight-gradient kernel, whose sums conv2d_gn_in's backward - which has
    #  no one-launch form - reproduces BIT for bit at 16 channels (tests/test_net_ops_gpu.py holds the pair to that).  The mixed pairs
    #  (csrc/conv_bwd_fused_mixed.hip) have the activation operand, written, with or without the sums)
    c16 = (cin, cout) != (32, 32)
    mixed_act = cin != cout and act == ACT_SELU and not accumulate and (sums is None or epi_act)
    fused = (gx is not None and split and BWD_FUSED and BF16X3 and cin in (16, 32) and cout in (16, 32) and cin_pad == cin and
             (k, pad) == (3, 1) and ((not keep_gpre or xgn is not None) if lz is not None else
                                     (xgn is None and (mixed_act if c16 else sums is None))))
    fkey = (cin, cout) if c16 else cin
    if fused and fkey not in _FUSED_WS:
        _FUSED_WS[fkey] = (lib.fn('dis_conv2d_bwd_fused_c16_workspace')(cin, cout) if c16 else
                           lib.fn('dis_conv2d_bwd_fused_workspace')(cin))
        if c16:
            _FUSED_WS['slots', cin, cout] = lib.fn('dis_conv2d_bwd_fused_c16_slots')(cin, cout)
    fused = fused and _FUSED_WS[fkey] >= 0
    # (the 16 -> 16 kernel runs two workgroups per CU: one slot of channel sums per workgroup)
    ab, slots = _gn_sums(n, cin, x.device, _FUSED_WS['slots', cin, cout] if fused and c16 else None) if epi or epi_act else (None, 0)
    ab_x, ab_act = sums if epi or epi_act else (None, None)
    acc = 1 if accumulate else 0

    def dgrad_done():
        if ab is not None and xgn is None:
            _GN_PRE[gx.data_ptr()] = (ab, slots)
        return after_dgrad(ab, slots) if after_dgrad is not None else None

    if lz is not None:
        _, g, q, coef, in_act = lz
        gpre = torch.empty_like(g) if keep_gpre else None
    else:
        g, q, coef, in_act, gpre = gy, (y if act != ACT_NONE else None), None, act, gy
    if fused:
        def launch(gw, gb):   # (gw may be the slice of a wider OIHW gradient, conv2d_multi: the slab reduce writes it in place)
            assert tuple(gw.stride()[1:]) == (9, 3, 1) and gw.stride(0) % 9 == 0
            st, gam, bet, eps = xgn if xgn is not None else (None, None, None, 0.0)
            ws = torch.empty(_FUSED_WS[fkey], dtype=torch.float32, device=x.device)
            if c16:
                return lib.call_try('dis_conv2d_bwd_fused_f16x2_c16', g, q, coef, in_act, gpre if lz is not None else None, weight,
                                    cout, cin, weight.stride(0), gx, acc, ab_x, ab_act, ab, slots, x, st, gam, bet, float(eps), gw, gb,
                                    ws, n, h, w, 0 if gw.is_contiguous() else gw.stride(0))
            return lib.call_try('dis_conv2d_bwd_fused_f16x2', g, q, coef, in_act, gpre if lz is not None else None, weight, cout, cin,
                                weight.stride(0), gx, acc, ab_x, ab_act, ab, x, st, gam, bet, float(eps), gw, gb, ws, n, h, w, cin,
                                0 if gw.is_contiguous() else gw.stride(0))
        ok, gw_ret, gb_ret = _into_sinks(weight, bias, grads, launch)
        if ok:
            return gpre, gw_ret, gb_ret, dgrad_done()
        if c16 and ab is not None:   # (no instance for this form: the two launches below take the slots of their own grid)
            ab, slots = _gn_sums(n, cin, x.device)
    # the same under the three-term split for the forms in BWD_FUSED_STRICT (dis_conv2d_bwd_fused_bf16x3, 32 -> 32): operand gy or
    # gy act'(y), x or GroupNorm(x); gx bit-identical to the input-gradient launch below
    form3 = 'xgn' if xgn is not None else ('act' if act != ACT_NONE else 'plain') + ('_accum' if accumulate else '')
    fused3 = (gx is not None and not split and BWD_FUSED and form3 in BWD_FUSED_STRICT and BF16X3 and cin == cout == cin_pad == 32 and
              (k, pad) == (3, 1) and lz is None and (xgn is None or (act == ACT_NONE and not accumulate)))
    if fused3 and cin not in _FUSED3_WS:
        _FUSED3_WS[cin] = lib.fn('dis_conv2d_bwd_fused_bf16x3_workspace')(cin)
    if fused3 and _FUSED3_WS[cin] >= 0:
        def launch3(gw, gb):
            assert tuple(gw.stride()[1:]) == (9, 3, 1) and gw.stride(0) % 9 == 0
            st, gam, bet, eps = xgn if xgn is not None else (None, None, None, 0.0)
            return lib.call_try('dis_conv2d_bwd_fused_bf16x3', g, q, in_act, weight, cout, cin, weight.stride(0), gx, acc, x, st, gam,
                                bet, float(eps), gw, gb, torch.empty(_FUSED3_WS[cin], dtype=torch.float32, device=x.device), n, h, w,
                                cin, 0 if gw.is_contiguous() else gw.stride(0))
        ok, gw_ret, gb_ret = _into_sinks(weight, bias, grads, launch3)
        if ok:
            return gpre, gw_ret, gb_ret, dgrad_done()
    after = None
    if lz is not None:
        gpre = torch.empty_like(g) if gpre is None else gpre
        if not lib.call_try('dis_conv2d_dgrad_f16x2_gnb', g, q, coef, in_act, gpre, weight, cout, cin, weight.stride(0), gx, acc,
                            ab_x, ab_act, ab, n, h, w, cin):
            # (no instance in this build: the pass as a launch of its own, then the forms of a plain operand)
            return _conv_bwd_slice(weight, x, gx, accumulate, grads, bias, pad, gy=_gn_lazy_materialize(lz), xgn=xgn, sums=sums,
                                   keep_gpre=keep_gpre, after_dgrad=after_dgrad)
        after = dgrad_done()
    elif gx is not None:
        kw = (n, gy.shape[1], gy.shape[2], cout, cin, k - 1 - pad)
        if act != ACT_NONE and ab is not None:
            lib.call('dis_conv2d_dgrad_bf16x3_act_gnsums_res', gy, y, weight, cout, cin, weight.stride(0), gx, ab_act, ab_x, ab, *kw)
        elif act != ACT_NONE:
            lib.call('dis_conv2d_dgrad_bf16x3_act', gy, y, act, weight, cout, cin, weight.stride(0), gx, *kw, acc)
        elif ab is not None and accumulate:
            lib.call('dis_conv2d_dgrad_bf16x3_gnsums_res', gy, weight, cout, cin, weight.stride(0), gx, ab_act, ab_x, ab, *kw)
        elif ab is not None:
            lib.call('dis_conv2d_dgrad_bf16x3_gnsums', gy, weight, cout, cin, weight.stride(0), gx, ab_x, ab, *kw)
        else:
            _conv_fwd_any(gy, weight, cin, 1, None, gx, None, n, gy.shape[1], gy.shape[2], cout, cin, k, 1, k - 1 - pad,
                          ACT_NONE | (CONV_ACCUM if accumulate else 0))
        after = dgrad_done()

    def wgrad(gw, gb):
        gwc = gw if gw.is_contiguous() else torch.empty(gw.shape, dtype=torch.float32, device=gw.device)
        wsz = lib.fn('dis_conv2d_wgrad_workspace')(cin_pad, cout, k, 1)
        if wsz < 0:
            raise lib.DisHipError(f'conv2d wgrad: unsupported shape cin={cin_pad} cout={cout} k={k}')
        ws = torch.empty(wsz, dtype=torch.float32, device=x.device)
        if xgn is not None:
            lib.call('dis_conv2d_wgrad_bf16x3_gn', x, *xgn, gpre, gwc, gb, ws, n, h, w, cin, cin, cout, k, 1, pad)
        elif act != ACT_NONE:
            lib.call('dis_conv2d_wgrad_bf16x3_act', x, gy, y, act, gwc, gb, ws, n, h, w, cin_pad, cin, cout, k, 1, pad)
        else:
            _conv_wgrad_any(x, gpre, gwc, gb, ws, n, h, w, cin_pad, cin, cout, k, 1, pad)
        if gwc is not gw:
            gw.copy_(gwc)   # (a small strided move into the slice of the wider gradient)
        return True
    _, gw_ret, gb_ret = _into_sinks(weight, bias, grads, wgrad)
    return gpre, gw_ret, gb_ret, after


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, act, want_stats, need_dgrad, gy_is_pre=False, join=None, gnres=None, pend=None):
        x, weight = _c(x), _c(weight)
        _chk(x, weight, bias)
        ctx.gnres = gnres
        n, hin, win, cin_pad = x.shape
        cout, cin, k, _ = weight.shape
        ho = (hin + 2 * pad - k) // stride + 1
        wo = (win + 2 * pad - k) // stride + 1
        y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
        stats = _zeros_d(2 * n, x.device) if want_stats else None
        if pend is not None:
            # x = SELU(GroupNorm(x2) + res) has not been written yet: this launch forms it on load and stores it (conv2d() checked
            # the shape; an unsupported mode falls back to the pass of its own)
            x2, gst, gam, bet, res, eps = pend
            if lib.call_try('dis_conv2d_fwd_f16x2_gnres', x2, gst, gam, bet, float(eps), res, x, weight, cout, cin, weight.stride(0),
                            bias, y, stats, n, hin, win, cin_pad, cout, act):
                _GN_PENDING.pop(x.data_ptr(), None)
            else:
                lib.call('dis_gn_apply', x2, gst, gam, bet, res, x, n, hin * win, cin_pad, ACT_SELU, float(eps))
                _GN_PENDING.pop(x.data_ptr(), None)
                _conv_fwd_any(x, weight, cin_pad, 0, bias, y, stats, n, hin, win, cin_pad, cout, k, stride, pad, act)
        else:
            _conv_fwd_any(x, weight, cin_pad, 0, bias, y, stats, n, hin, win, cin_pad, cout, k, stride, pad, act)
        if gy_is_pre:
            act = ACT_NONE  # the consumer (group_norm(in_act=...)) hands back the pre-activation gradient
        ctx.save_for_backward(x, weight, y if act != ACT_NONE else None)
        ctx.cfg = (stride, pad, act, bias is not None, need_dgrad)
        ctx.bias_ref = bias  # only its address/shape are used (gradient sink lookup)
        ctx.join = join
        return _with_stats(ctx, y, stats)

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, weight, y = ctx.saved_tensors
        stride, pad, act, has_bias, need_dgrad = ctx.cfg
        n, hin, win, cin_pad = x.shape
        cout, cin, k, _ = weight.shape
        join = ctx.join or _SOLE
        want_gx = need_dgrad and ctx.needs_input_grad[0]
        # a token of a GroupNorm behind this conv (ops._GN_LAZY): its backward's elementwise pass is applied by this conv's
        # input-gradient launch on load, which also writes the values for the weight-gradient launch
        lz = _gn_lazy_pop(gy, ctx)
        gw_ret = gb_ret = None
        wdone = False
        if lz is not None and (stride != 1 or act != ACT_NONE):
            if (act == ACT_NONE and _gn_lazy_k4s2(cin_pad, cin, cout, k, stride, pad) and lib.fn('dis_get_conv_split')() == 1 and
                    x[0].numel() * 4 < 0x7fff0000):   # (the kernel's per-sample 31-bit offsets)
                # the 4 x 4 stride-2 down convolution: the WEIGHT-gradient launch applies the pass while it stages gy (no halo there)
                # and stores the values for the four parity launches of the input gradient below
                _, lg, lq, lcoef, lin_act = lz
                gpre = torch.empty_like(lg)
                ws = torch.empty(lib.fn('dis_conv2d_wgrad_workspace')(cin_pad, cout, k, stride), dtype=torch.float32, device=x.device)
                ok, gw_ret, gb_ret = _into_sinks(weight, ctx.bias_ref, None, lambda gw, gb: lib.call_try(
                    'dis_conv2d_wgrad_k4s2_f16x2_gnb', x, lg, lq, lcoef, lin_act, gpre, gw, gb, ws, n, hin, win))
                if ok:
                    gy, lz, wdone = gpre, None, True
            # (no instance for this configuration in this build - e.g. an input activation the kernel has no form for: the pass
            #  runs as a launch of its own, the general path below does the rest)
            if lz is not None:
                gy, lz = _gn_lazy_materialize(lz), None
        if lz is None:
            gy = _c(gy)
        gpre = gy
        # bf16x3 shapes: the activation gradient is applied while gy is staged (dgrad and wgrad kernels), no separate pass
        fuse_act = act != ACT_NONE and _bx_shape(cin_pad, cout, k, stride)
        # the 4 -> 16 stems (conv1, amb_conv): no input gradient is asked for, so gy act'(y) would be formed for the weight-gradient
        # launch alone - that launch forms it on load (dis_conv2d_wgrad_act), the pass (read gy, y; write gpre) does not exist
        wgrad_act = (act != ACT_NONE and not fuse_act and not want_gx and cin_pad == 4 and cout == 16 and
                     (k, stride) in ((3, 1), (4, 2)))
        if act != ACT_NONE and not fuse_act and not wgrad_act:
            gpre = torch.empty_like(gy)
            lib.call('dis_act_bwd', gy, y, gpre, act, gy.numel())
        if want_gx:
            assert cin_pad == cin
        gx = None
        if stride != 1 or wgrad_act:
            # the 4 x 4 stride-2 convolutions and the 4 -> 16 stems
            if want_gx:
                gx, second = join.target(x)
                _dgrad_k4s2(gpre, weight, gx, n, hin, win, cin, cout, second)
                gx = join.result(gx, second)
            if not wdone:
                gw, gw_ret = _sink(weight)
                gb, gb_ret = _sink_opt(ctx.bias_ref)
                wsz = lib.fn('dis_conv2d_wgrad_workspace')(cin_pad, cout, k, stride)
                if wsz < 0:
                    raise lib.DisHipError(f'conv2d wgrad: unsupported shape cin={cin_pad} cout={cout} k={k} s={stride}')
                ws = torch.empty(wsz, dtype=torch.float32, device=x.device)
                if wgrad_act and not lib.call_try('dis_conv2d_wgrad_act', x, gy, y, act, gw, gb, ws, n, hin, win, cin_pad, cin, cout,
                                                  k, stride, pad):
                    gpre = torch.empty_like(gy)   # (no instance in this build: the pass as a launch of its own)
                    lib.call('dis_act_bwd', gy, y, gpre, act, gy.numel())
                    wgrad_act = False
                if not wgrad_act:
                    _conv_wgrad_any(x, gpre, gw, gb, ws, n, hin, win, cin_pad, cin, cout, k, stride, pad)
            _sinks_written()
            return gx, gw_ret, gb_ret, None, None, None, None, None, None, None, None, None
        gnres = ctx.gnres
        sums = None
        if (want_gx and fuse_act and gnres is not None and ctx.join is None and act == ACT_SELU and (GN_SUMS & 1) and
                (cout, cin) == (16, 32) and tuple(gnres[0].shape) == tuple(x.shape) and lib.fn('dis_get_conv_split')() == 1):
            # final_conv: x = SELU(GroupNorm(.) + res) of ref_res3 and this conv is its only consumer - its input gradient is written
            # times SELU'(x) and its launch leaves that GroupNorm's backward sums (as the residual form below)
            sums = (gnres[0], x)
        tgt, second = join.target(x) if want_gx else (None, False)
        # x is out = SELU(GroupNorm(x2) + res) of the previous ResNetBlock (gnres = (x2,)), or GroupNorm(x2) with two consumers
        # (gnres = (x2, None)), and gx - which arrives holding the other consumer's gradient - becomes the complete gradient wrt out
        # here: the epilogue turns it into the gradient wrt the pre-activation value (times SELU'(x)) and leaves the
        # GroupNorm-backward sums, so that GroupNorm's backward needs neither its reduce pass nor a residual-gradient write
        if second and gnres is not None and (GN_SUMS & 2) and tuple(gnres[0].shape) == tuple(x.shape):
            sums = (gnres[0], x if len(gnres) == 1 else None)
        _, gw_ret, gb_ret, _ = _conv_bwd_slice(weight, x, tgt, second, bias=ctx.bias_ref, pad=pad, lz=lz, gy=gy if fuse_act else gpre,
                                               act=act if fuse_act else ACT_NONE, y=y, sums=sums)
        if tgt is not None:
            gx = join.result(tgt, second)
        _sinks_written()
        return gx, gw_ret, gb_ret, None, None, None, None, None, None, None, None, None


def conv2d(x, weight, bias, stride=1, pad=0, act=ACT_NONE, want_stats=False, need_dgrad=True, gy_is_pre=False,
           join=None, gnres=None):
    """x nhwc (n,h,w,cin_pad>=cin); weight OIHW.  Returns (y, stats|None).
    gy_is_pre: the only consumer of y is group_norm(..., in_act=act), whose backward already multiplies by act'(y);
    the incoming gradient is then taken as the pre-activation gradient.
    join: GradJoin shared with the other consumer of x (see GradJoin)."""
    pend = getattr(x, '_pending_gn', None)
    if pend is not None:
        cout_, cin_, k_, _ = weight.shape
        if not (k_ == 3 and stride == 1 and pad == 1 and act == ACT_SELU and x.shape[-1] == cin_ and BF16X3 and
                ((cin_ == cout_ and cin_ in (16, 32)) or ((cin_, cout_) == (32, 16) and not want_stats))):
            realize(x)
            pend = None
        else:
            x._pending_gn = None   # (written by the launch below)
    out = _Conv2d.apply(x, weight, bias, stride, pad, act, want_stats, need_dgrad, gy_is_pre, join, gnres, pend)
    if (act == ACT_NONE or gy_is_pre) and ((need_dgrad and _gn_lazy_shape(x.shape[-1], weight.shape[0], weight.shape[2], stride, pad)) or
                                           _gn_lazy_k4s2(x.shape[-1], weight.shape[1], weight.shape[0], weight.shape[2], stride, pad)):
        _mark_lazy_ok(out)   # (a GroupNorm that is this output's ONLY consumer may answer with a token, see _GN_LAZY)
    return out


GN_FUSE = _os.environ.get('DIS_GN_FUSE', '1') != '0'
# GroupNorm backward from the sums of the input-gradient epilogue.  DIS_GN_SUMS=0 disables it; as a bit mask (diagnostics) it selects
# the forms: 1 final_conv (activation + residual), 2 residual / two-consumer, 4 GroupNorm-on-load pairs, 8 conv_fuse's first slice
GN_SUMS = int(_os.environ.get('DIS_GN_SUMS', '15'))


def gn_fusable(cin, cout, k, stride):
    """conv2d_gn_in exists for the bf16x3 square shapes (3x3, stride 1, 16 -> 16 / 32 -> 32)"""
    return GN_FUSE and BF16X3 and cin == cout and cin in (16, 32) and k == 3 and stride == 1


def _gn_bwd_from_sums(g, x, stats, gamma, ab, slots, gg, gb, eps, in_act, uid):
    """GroupNorm(1 group) backward from the channel sums an earlier launch left (ab): a token when the producer of x redeems one
    (uid, _GN_LAZY), else one elementwise pass.  -> gradient wrt x"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    if uid and GN_LAZY:
        return _gn_lazy_defer(g, x, stats, gamma, ab, slots, gg, gb, n, hw, c, eps, in_act, uid=uid)
    gx = torch.empty_like(x)
    lib.call('dis_gn_bwd_from_sums', g, x, stats, gamma, ab, slots, gx, gg, gb, _gn_coef(n, c, x.device), n, hw, c, eps, in_act)
    return gx


def _gn_apply_bwd(g, y, x, stats, gamma, gres, gg, gb, act, eps, in_act):
    """GroupNorm(1 group) backward as a reduce and an apply launch over g (and y, x).  -> gradient wrt x"""
    n, c = x.shape[0], x.shape[-1]
    gx = torch.empty_like(x)
    wtot = lib.fn('dis_gn_bwd_workspace')(n, c)
    ws = torch.empty(wtot, dtype=torch.float64, device=x.device)
    nred2 = wtot // (2 + 2 * c) * 2  # (n * blocks-per-sample-max) pairs of per-block sums, then the parameter partials
    lib.call('dis_gn_apply_bwd', g, y, x, stats, gamma, gx, gres, gg, gb, ws[:nred2], ws[nred2:], n, x.numel() // (n * c), c, act,
             eps, in_act)
    return gx


def _gn_bwd_after_dgrad(g, x, stats, gamma, beta, eps, in_act, ab, slots, uid):
    """The backward of a GroupNorm that a conv applied on load (conv2d_gn_in), once that conv's input gradient g exists: from the
    channel sums its launch left (ab), else the reduce and apply launches.  -> (gradient wrt x, gamma's and beta's for autograd)"""
    gg, gg_ret = _sink(gamma)
    gb, gb_ret = _sink(beta)
    if ab is not None:
        return _gn_bwd_from_sums(g, x, stats, gamma, ab, slots, gg, gb, eps, in_act, uid), gg_ret, gb_ret
    return _gn_apply_bwd(g, None, x, stats, gamma, None, gg, gb, ACT_NONE, eps, in_act), gg_ret, gb_ret


class _Conv2dGnIn(torch.autograd.Function):
    """y = act(conv3x3(GroupNorm(x)) + bias) where the GroupNorm (1 group; its statistics `gn_stats` come from the epilogue of
    the conv that produced x) is applied by the conv kernels while they stage x: the normalised tensor is never written or
    read (reference: the conv -> SELU -> GroupNorm -> conv chains of ResNetBlock / Block2D3D, model/multi_frame_networks.py
    :338-345,:514-542).  One autograd node for the pair GroupNorm + conv: its backward runs the conv's input gradient, the
    GroupNorm backward (which hands the producer of x its PRE-activation gradient when `in_act` is that producer's
    activation) and the conv's weight gradient with the same on-load normalisation."""

    @staticmethod
    def forward(ctx, x, gn_stats, gamma, beta, weight, bias, pad, act, want_stats, gy_is_pre, eps, in_act, x_lazy=False):
        ctx.x_lazy = x_lazy   # the producer of x redeems a token for the GroupNorm's elementwise backward pass (_GN_LAZY)
        x, weight = _c(x), _c(weight)
        _chk(x, gamma, beta, weight, bias)
        n, h, w, cin = x.shape
        cout, _, k, _ = weight.shape
        assert gn_fusable(cin, cout, k, 1) and weight.shape[1] == cin
        ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
        y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
        stats = _zeros_d(2 * n, x.device) if want_stats else None
        lib.call('dis_conv2d_fwd_bf16x3_gn', x, gn_stats, gamma, beta, float(eps), weight, cout, cin, weight.stride(0), bias, y,
                 stats, n, h, w, cin, cout, k, 1, pad, act)
        if gy_is_pre:
            act = ACT_NONE
        ctx.save_for_backward(x, gn_stats, gamma, weight, y if act != ACT_NONE else None)
        ctx.cfg = (pad, act, bias is not None, float(eps), in_act)
        ctx.bias_ref, ctx.beta_ref = bias, beta
        return _with_stats(ctx, y, stats)

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, gn_stats, gamma, weight, y = ctx.saved_tensors
        pad, act, has_bias, eps, in_act = ctx.cfg
        # (this conv's own output gradient may be a token of the GroupNorm behind it: redeemed by the input-gradient launch)
        lz = _gn_lazy_pop(gy, ctx)
        if lz is not None and act != ACT_NONE:
            gy, lz = _gn_lazy_materialize(lz), None
        gpre = gy
        if lz is None:
            gy = gpre = _c(gy)
            if act != ACT_NONE:   # (not the case in the networks here: the consumers are followed by a GroupNorm themselves)
                gpre = torch.empty_like(gy)
                lib.call('dis_act_bwd', gy, y, gpre, act, gy.numel())
        # gradient wrt the normalised tensor (the input-gradient launch leaves the per-(sample, channel) sums of g and g * x in
        # its epilogue), then through the GroupNorm to the producer's (pre-activation) output
        gnorm = torch.empty_like(x)
        _, gw_ret, gb_ret, (gx, gg_ret, gbt_ret) = _conv_bwd_slice(
            weight, x, gnorm, False, bias=ctx.bias_ref, pad=pad, lz=lz, gy=gpre, xgn=(gn_stats, gamma, ctx.beta_ref, eps),
            sums=(x, None) if GN_SUMS & 4 else None,
            after_dgrad=lambda ab, slots: _gn_bwd_after_dgrad(gnorm, x, gn_stats, gamma, ctx.beta_ref, eps, in_act, ab, slots,
                                                              ctx.x_lazy))
        _sinks_written()
        return gx, None, gg_ret, gbt_ret, gw_ret, gb_ret, None, None, None, None, None, None, None


def conv2d_gn_in(x, gn_stats, gamma, beta, weight, bias, pad=1, act=ACT_NONE, want_stats=False, gy_is_pre=False, eps=1e-5,
                 in_act=ACT_NONE):
    """conv2d(group_norm(x, gamma, beta, stats=gn_stats, in_act=in_act), weight, bias, 1, pad, act, ...) with the
    normalisation applied on load.  Returns (y, stats|None).  Shapes: see gn_fusable()."""
    out = _Conv2dGnIn.apply(x, gn_stats, gamma, beta, weight, bias, pad, act, want_stats, gy_is_pre, eps, in_act,
                            int(getattr(x, '_gn_lazy_ok', 0)))
    if (act == ACT_NONE or gy_is_pre) and _gn_lazy_shape(x.shape[-1], weight.shape[0], weight.shape[2], 1, pad):
        _mark_lazy_ok(out)
    return out


class _Conv2dMulti(torch.autograd.Function):
    """Conv2d (stride 1) over the channel concatenation of several nhwc tensors WITHOUT materialising the
    concatenation: one launch per source with the matching slice of the weight, the later launches accumulate into
    y (DIS_CONV_ACCUM); bias enters with the first launch, the activation and the GroupNorm statistics with the last.
    The backward produces one input gradient per source directly (no split copies).
    gn_*: the FIRST source is the input of a GroupNorm that is applied on load (see _Conv2dGnIn): xs[0] is the pre-normalisation
    tensor, gn_meta = (eps, in_act); its GroupNorm backward runs inside this node (sums in the input-gradient epilogue)."""

    @staticmethod
    def forward(ctx, weight, bias, pad, act, want_stats, gy_is_pre, gn_stats, gn_gamma, gn_beta, gn_meta, *xs):
        ctx.x0_lazy = int(gn_meta[2]) if (gn_meta is not None and len(gn_meta) > 2 and gn_meta[2]) else 0   # (uid of xs[0]'s producer)
        gn_meta = gn_meta[:2] if gn_meta is not None else None
        # (tokens of a GroupNorm behind this conv are redeemed by the first source's 3 x 3 c -> c input-gradient launch)
        ctx.lazy_ok = _multi_lazy_ok(weight, xs, pad, act)
        # a source that is SELU(GroupNorm(x2) + residual) of a ResNetBlock and has no other consumer: its input-gradient launch
        # leaves that GroupNorm's backward sums (as _Conv2d.backward does for final_conv)
        ctx.gnres = [getattr(x, '_gn_res_src', None) if x.requires_grad else None for x in xs]
        xs = [_c(x) for x in xs]
        weight = _c(weight)
        _chk(weight, bias, *xs)
        cout, cin, k, _ = weight.shape
        n, h, w, _ = xs[0].shape
        cs = [x.shape[3] for x in xs]
        assert sum(cs) == cin and all(tuple(x.shape[:3]) == (n, h, w) for x in xs)
        ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
        y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=weight.device)
        stats = _zeros_d(2 * n, weight.device) if want_stats else None
        off = 0
        for i, x in enumerate(xs):
            last = i == len(xs) - 1
            wi = weight[:, off:off + cs[i]]  # a view: no copy
            a = (act if last else ACT_NONE) | (CONV_ACCUM if i > 0 else 0)
            if i == 0 and gn_meta is not None:
                assert gn_fusable(cs[0], cout, k, 1) and len(xs) > 1
                lib.call('dis_conv2d_fwd_bf16x3_gn', x, gn_stats, gn_gamma, gn_beta, float(gn_meta[0]), wi, cout, cs[0],
                         wi.stride(0), bias, y, None, n, h, w, cs[0], cout, k, 1, pad, ACT_NONE)
            else:
                _conv_fwd_any(x, wi, cs[i], 0, bias if i == 0 else None, y, stats if last else None, n, h, w, cs[i], cout, k, 1,
                              pad, a)
            off += cs[i]
        if gy_is_pre:
            act = ACT_NONE
        ctx.save_for_backward(weight, y if act != ACT_NONE else None, gn_stats, gn_gamma, *xs)
        ctx.cfg = (pad, act, bias is not None, cs, gn_meta)
        ctx.bias_ref, ctx.beta_ref = bias, gn_beta
        return _with_stats(ctx, y, stats)

    @staticmethod
    def backward(ctx, gy, _gstats):
        weight, y, gn_stats, gn_gamma = ctx.saved_tensors[:4]
        xs = ctx.saved_tensors[4:]
        pad, act, has_bias, cs, gn_meta = ctx.cfg
        cout, cin, k, _ = weight.shape
        n, h, w, _ = xs[0].shape
        fuse_act = act != ACT_NONE and all(_bx_shape(c_, cout, k, 1) for c_ in cs)  # see _Conv2d.backward
        assert gn_meta is None or act == ACT_NONE
        # this conv's output gradient may be a token of the GroupNorm behind it (conv_fuse): the FIRST source's input-gradient launch
        # applies the elementwise pass on load and stores the result for every other launch of this node
        lz = _gn_lazy_pop(gy, ctx)
        if lz is not None and act != ACT_NONE:
            gy, lz = _gn_lazy_materialize(lz), None
        gpre = gy
        if lz is None:
            gy = gpre = _c(gy)
            if act != ACT_NONE and not fuse_act:
                gpre = torch.empty_like(gy)
                lib.call('dis_act_bwd', gy, y, gpre, act, gy.numel())
        gw, gw_ret = _sink(weight)
        gb, gb_ret = _sink_opt(ctx.bias_ref)
        gg_ret = gbt_ret = None
        gxs = []
        off = 0
        for i, x in enumerate(xs):
            wi = weight[:, off:off + cs[i]]  # a view: no copy
            grads = (gw[:, off:off + cs[i]], gb if i == 0 else None)   # (the fused launch writes the slice in place)
            gx = torch.empty_like(x) if ctx.needs_input_grad[10 + i] else None
            gnres = ctx.gnres[i]
            if i == 0 and gn_meta is not None:
                # gradient wrt the normalised tensor, then through the GroupNorm (as _Conv2dGnIn.backward)
                eps, in_act = float(gn_meta[0]), gn_meta[1]
                gnorm = torch.empty_like(x) if gx is not None else None
                gpre, _, _, gn = _conv_bwd_slice(
                    wi, x, gnorm, False, grads, pad=pad, lz=lz, gy=gpre, xgn=(gn_stats, gn_gamma, ctx.beta_ref, eps),
                    sums=(x, None) if GN_SUMS & 8 else None, keep_gpre=True,
                    after_dgrad=lambda ab, slots: _gn_bwd_after_dgrad(gnorm, x, gn_stats, gn_gamma, ctx.beta_ref, eps, in_act, ab, slots,
                                                                      ctx.x0_lazy))
                if gn is not None:
                    gx, gg_ret, gbt_ret = gn
            elif (gx is not None and fuse_act and act == ACT_SELU and gnres is not None and (GN_SUMS & 1) and (cout, cs[i]) == (32, 16) and
                  k == 3 and pad == 1 and tuple(gnres[0].shape) == tuple(x.shape) and lib.fn('dis_get_conv_split')() == 1):
                # (x = SELU(GroupNorm(.) + res) of a ResNetBlock and this slice is its only consumer: as final_conv in _Conv2d.backward)
                _conv_bwd_slice(wi, x, gx, False, grads, pad=pad, gy=gy, act=act, y=y, sums=(gnres[0], x))
            else:
                gpre_i = _conv_bwd_slice(wi, x, gx, False, grads, pad=pad, lz=lz, gy=gy if fuse_act else gpre,
                                         act=act if fuse_act else ACT_NONE, y=y, keep_gpre=True)[0]
                gpre = gpre if fuse_act else gpre_i
            lz = None   # (redeemed or materialised by the first source's launch)
            gxs.append(gx)
            off += cs[i]
        _sinks_written()
        return (gw_ret, gb_ret, None, None, None, None, None, gg_ret, gbt_ret, None) + tuple(gxs)


def _multi_lazy_ok(weight, xs, pad, act):
    cout, _, k, _ = weight.shape
    return bool(act == ACT_NONE and xs[0].requires_grad and xs[0].shape[-1] == cout and _gn_lazy_shape(cout, cout, k, 1, pad))


def conv2d_multi(xs, weight, bias, pad=0, act=ACT_NONE, want_stats=False, gy_is_pre=False, gn0=None):
    """conv2d(cat(xs, channel dim), weight) without the cat.  Returns (y, stats|None).
    gn0 = (stats, gamma, beta, eps, in_act): xs[0] is the INPUT of a GroupNorm(1 group) that is applied on load (conv2d_gn_in)."""
    if gn0 is not None:
        out = _Conv2dMulti.apply(weight, bias, pad, act, want_stats, gy_is_pre, gn0[0], gn0[1], gn0[2],
                                 (gn0[3], gn0[4], int(getattr(xs[0], '_gn_lazy_ok', 0))), *xs)
    else:
        out = _Conv2dMulti.apply(weight, bias, pad, act, want_stats, gy_is_pre, None, None, None, None, *xs)
    if _multi_lazy_ok(weight, xs, pad, act):
        _mark_lazy_ok(out)   # (a GroupNorm that is this output's ONLY consumer may answer with a token, see _GN_LAZY)
    return out


# DIS_MF_BWD_FUSED=0: conv_mf's backward as two launches (input gradient with the stored operand, then the weight gradient) (A/B)
MF_BWD_FUSED = _os_env.environ.get('DIS_MF_BWD_FUSED', '1') != '0'


class _Conv2dScaledIn(torch.autograd.Function):
    """y = conv2d(x * xscale[..., chunk]) with the multiplier applied inside the kernels: forward while the input is
    staged, input gradient in the epilogue (optionally accumulating into a GradJoin buffer), weight gradient while x
    is staged.  x (n,h,w,cin), xscale (n,h,w,cin/32)."""

    @staticmethod
    def forward(ctx, x, xscale, weight, bias, stride, pad, act, want_stats, join):
        x, xscale, weight = _c(x), _c(xscale), _c(weight)
        _chk(x, xscale, weight, bias)
        n, hin, win, cin = x.shape
        cout, _, k, _ = weight.shape
        assert cin % 32 == 0 and tuple(xscale.shape) == (n, hin, win, cin // 32) and act == ACT_NONE
        ho, wo = (hin + 2 * pad - k) // stride + 1, (win + 2 * pad - k) // stride + 1
        y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
        stats = _zeros_d(2 * n, x.device) if want_stats else None
        lib.call('dis_conv2d_fwd_scaled', x, xscale, _pack_w(weight, cin, 0), bias, y, None, stats, n, hin, win, cin, cout,
                 k, stride, pad, act)
        ctx.save_for_backward(x, xscale, weight)
        ctx.cfg = (stride, pad, bias is not None)
        ctx.bias_ref = bias
        ctx.join = join
        return _with_stats(ctx, y, stats)

    @staticmethod
    def backward(ctx, gy, _gstats):
        x, xscale, weight = ctx.saved_tensors
        stride, pad, has_bias = ctx.cfg
        n, hin, win, cin = x.shape
        cout, _, k, _ = weight.shape
        # (a token of the GroupNorm behind this conv, ops._GN_LAZY: the 1 x 1 input-gradient launch applies the pass on load)
        lz = _gn_lazy_pop(gy, ctx)
        if lz is not None and not (ctx.needs_input_grad[0] and k == 1 and stride == 1 and pad == 0 and (cin, cout) == (128, 32)):
            gy, lz = _gn_lazy_materialize(lz), None
        gx = None
        join = ctx.join or _SOLE
        gw, gw_ret = _sink(weight)
        gb, gb_ret = _sink(ctx.bias_ref) if has_bias else (None, None)
        if lz is not None:
            _, lg, lq, lcoef, lin_act = lz
            gx, second = join.target(x)
            # one launch for both gradients (csrc/conv1x1_bwd_fused.hip): the operand act'(q) (g k1 + q kx + k0) stays in LDS
            wsz = lib.fn('dis_conv2d_bwd1x1_scaled_gnb_workspace')(cin, cout) if MF_BWD_FUSED else -1
            if wsz >= 0 and lib.call_try('dis_conv2d_bwd1x1_scaled_gnb', lg, lq, lcoef, lin_act, _pack_w(weight, cin, 1), gx, xscale, x,
                                         xscale, gw, gb, torch.empty(wsz, dtype=torch.float32, device=x.device), n, hin, win,
                                         cout, cin, 1 if second else 0):
                _sinks_written()
                return join.result(gx, second), None, gw_ret, gb_ret, None, None, None, None, None
            gy = torch.empty_like(lg)
            lib.call('dis_conv2d_dgrad1x1_scaled_gnb', lg, lq, lcoef, lin_act, gy, _pack_w(weight, cin, 1), gx, xscale, n, hin, win,
                     cout, cin, 1 if second else 0)
            gx = join.result(gx, second)
        gy = _c(gy)
        if lz is None and ctx.needs_input_grad[0]:
            assert stride == 1
            gx, second = join.target(x)
            lib.call('dis_conv2d_fwd_scaled', gy, None, _pack_w(weight, cin, 1), None, gx, xscale, None, n, gy.shape[1],
                     gy.shape[2], cout, cin, k, 1, k - 1 - pad, ACT_NONE | (CONV_ACCUM if second else 0))
            gx = join.result(gx, second)
        wsz = lib.fn('dis_conv2d_wgrad_workspace')(cin, cout, k, stride)
        ws = torch.empty(wsz, dtype=torch.float32, device=x.device)
        lib.call('dis_conv2d_wgrad_scaled', x, xscale, gy, gw, gb, ws, n, hin, win, cin, cin, cout, k, stride, pad)
        _sinks_written()
        return gx, None, gw_ret, gb_ret, None, None, None, None, None


def conv2d_scaled_in(x, xscale, weight, bias, stride=1, pad=0, want_stats=False, join=None):
    out = _Conv2dScaledIn.apply(x, xscale, weight, bias, stride, pad, ACT_NONE, want_stats, join)
    if GN_LAZY and weight.shape[2] == 1 and stride == 1 and pad == 0 and (x.shape[-1], weight.shape[0]) == (128, 32):
        _mark_lazy_ok(out)   # (its backward redeems GroupNorm tokens: dis_conv2d_dgrad1x1_scaled_gnb)
    return out


def slot_weights(geom):
    """(tl,bs,h,w,tl,4) geometry -> (tl*bs,h,w,tl) multipliers mask/mean(mask) (reference multi_frame_networks.py:410)"""
    geom = _c(geom)
    tl, bs, h, w, s, _ = geom.shape
    out = torch.empty((tl * bs, h, w, s), dtype=torch.float32, device=geom.device)
    lib.call('dis_slot_weights', geom, out, tl * bs * h * w, s)
    return out


class _DispHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, alpha, offset):
        x, weight, bias = _c(x), _c(weight), _c(bias)
        _chk(x, weight, bias)
        n, h, w, cin = x.shape
        y = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device)
        lib.call('dis_disp_head_fwd', x, weight, bias, y, n, h, w, cin, float(alpha), float(offset))
        ctx.save_for_backward(x, weight, y)
        ctx.alpha = float(alpha)
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        n, h, w, cin = x.shape
        gx = torch.empty_like(x)
        gw, gw_ret = _sink(weight)
        gb, gb_ret = _sink(ctx.bias_ref)
        ws = torch.empty(lib.fn('dis_disp_head_bwd_workspace')(n, h, w, cin), dtype=torch.float32, device=x.device)
        lib.call('dis_disp_head_bwd', x, weight, y, _c(gy), gx, gw, gb, ws, n, h, w, cin, ctx.alpha)
        _sinks_written()
        return gx, gw_ret, gb_ret, None, None


def disp_head(x, weight, bias, alpha, offset=3.0):
    return _DispHead.apply(x, weight, bias, alpha, offset)


# --------------------------------------------------------------------------------------------------
# general convolution family (DIS-SF / DispNetS): streaming implicit GEMM, csrc/conv_gen.hip
# --------------------------------------------------------------------------------------------------
CONVG_CONV, CONVG_CONV_DGRAD, CONVG_TCONV, CONVG_TCONV_DGRAD = 0, 1, 2, 3


def _ld(t):
    """pixel stride (floats) of an nhwc tensor that is dense or a channel range of a wider dense nhwc buffer
    (ConcatBuf.slot), None for any other layout"""
    if t.dim() == 4 and t.is_contiguous():
        return t.shape[3]
    if t.dim() != 4 or t.stride(3) != 1:
        return None
    ld = t.stride(2)
    n, h, w, c = t.shape
    if (ld < c or ld % 4 or t.stride(1) != w * ld or t.stride(0) != h * w * ld or t.data_ptr() % 16):
        return None
    return ld


def _nhwc(t):
    """t as the kernels can address it: itself if _ld(t) applies, else a dense copy"""
    return t if _ld(t) is not None else t.contiguous()


class ConcatBuf(object):
    """Channel concatenation without the copy (the reference concatenates decoder inputs with torch.cat,
    model/networks.py:262-288): ONE nhwc buffer per concatenation, zero-padded to a multiple of 4 channels; every
    producer writes its channel range in place (convg(..., out=buf.slot(off, c)), write_channels) and hands the range
    on as an ordinary tensor (a view); joined(parts) returns the whole buffer as the consumer's input and routes the
    gradient ranges back to the parts.  All writes go through the C ABI, never through ATen in-place ops: the views
    saved for backward keep their version."""

    def __init__(self, n, h, w, c, device, dtype=torch.float32):
        self.c = c
        q = 8 if dtype == torch.bfloat16 else 4   # 16-byte vectors: 4 floats / 8 bf16
        ld = (c + q - 1) // q * q
        self.q = q
        self.buf = torch.empty((n, h, w, ld), dtype=dtype, device=device)
        self.pad = ld - c  # zero lanes behind the last channel: written together with it (write_channels)

    def slot(self, off, c):
        assert off % self.q == 0 and off + c <= self.c
        return (self.buf, off, c)

    def joined(self, parts):
        """parts: [(tensor written into the buffer, channel offset)]"""
        return _CatFrom.apply(self, tuple(o for _, o in parts), *[p for p, _ in parts])


class _CatFrom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cbuf, offs, *parts):
        ctx.offs = offs
        ctx.cs = tuple(p.shape[3] for p in parts)
        return cbuf.buf.view(cbuf.buf.shape)

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(g[..., o:o + c] for o, c in zip(ctx.offs, ctx.cs))


# --------------------------------------------------------------------------------------------------
# The streaming convolutions of DispNetS for two activation storages: fp32 (csrc/conv_gen.hip), and bf16 (BASELINE config 2;
# csrc/conv_bf16.hip): nhwc feature maps are torch.bfloat16 - one bf16 product per MAC, fp32 accumulation - while parameters,
# parameter gradients and disparities stay float32.  One autograd path serves both; a _Storage carries what differs.
# --------------------------------------------------------------------------------------------------
BF16 = torch.bfloat16


def _isbf(t):
    return 1 if t.dtype == BF16 else 0


def _chk_f32(x):
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError('depthinspace_amd ops need float32 CUDA(HIP) tensors: the HIP path is the only path')


def _chk_act(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda or t.dtype not in (torch.float32, BF16):
            raise RuntimeError('depthinspace_amd bf16 ops need float32 / bfloat16 CUDA(HIP) tensors: the HIP path is the only path')
        if _ld(t) is None or (t.dtype == BF16 and _ld(t) % 8):
            raise RuntimeError('expected a dense nhwc tensor or a channel range of one (bf16: channels in multiples of 8)')


def _convg_run(mode, x, w, bias, y, n, hin, win, cin, cin_w, hout, wout, cout, cout_w, k, stride, pad, act):
    per = lib.fn('dis_convg_pack_workspace')(cin, cout, k)
    if per < 0:
        raise lib.DisHipError(f'convg: unsupported shape cin={cin} cout={cout} k={k}')
    phases = 4 if (mode in (CONVG_CONV_DGRAD, CONVG_TCONV) and stride == 2) else 1
    sk = lib.fn('dis_convg_splitk_workspace')(mode, n, hin, win, hout, wout, cin, cout, k, stride, pad)   # (small maps: split-K partials)
    wp = torch.empty(per * phases + max(sk, 0), dtype=torch.float32, device=x.device)
    lib.call('dis_convg_run', mode, x, _ld(x), 0, w, bias, y, _ld(y), 0, wp, n, hin, win, cin, cin_w, hout,
             wout, cout, cout_w, k, stride, pad, act)


CONVB_PREPACKED = 0x100   # include/dis_hip.h DIS_CONVB_PREPACKED


def _convb_run(mode, x, w, bias, y, n, hin, win, cin, cin_w, hout, wout, cout, cout_w, k, stride, pad, act):
    per = lib.fn('dis_convb_pack_workspace')(cin, cout, k)
    if per < 0:
        raise lib.DisHipError(f'convb: unsupported shape cin={cin} cout={cout} k={k}')
    sk = lib.fn('dis_convb_splitk_workspace')(mode, _isbf(x), n, hin, win, hout, wout, cin, cout, k, stride, pad)   # floats
    key = (w.data_ptr(), mode, _isbf(x), _isbf(y), n, hin, win, cin, cin_w, hout, wout, cout, cout_w, k, stride, pad)
    wp, prepacked = _PackBatch.workspace(key, per * 4 + 2 * max(sk, 0), x.device, w)
    ldy = y.stride(2) if y.dim() == 4 else 1
    lib.call('dis_convb_run', mode | (CONVB_PREPACKED if prepacked else 0), x, _isbf(x), _ld(x), 0, w, bias, y, _isbf(y), ldy, 0,
             wp, n, hin, win, cin, cin_w, hout, wout, cout, cout_w, k, stride, pad, act)


def _wgrad(entry, X, hX, wX, cX, cX_w, G, hG, wG, cG, cG_w, gw, n, k, stride, pad):
    """weight gradient through `entry` = dis_convg_wgrad (fp32 operands) or dis_convb_wgrad (each operand fp32 or bf16: it takes their
    storage flags)"""
    wsz = lib.fn(entry + '_workspace')(n, hG, wG, cX, cG, k)
    if wsz < 0:
        raise lib.DisHipError(f'{entry}: unsupported shape')
    ws = torch.empty(wsz, dtype=torch.float32, device=X.device)
    fx, fg = ((_isbf(X),), (_isbf(G),)) if entry == 'dis_convb_wgrad' else ((), ())
    lib.call(entry, X, *fx, _ld(X), 0, hX, wX, cX, cX_w, G, *fg, _ld(G), 0, hG, wG, cG, cG_w, gw, ws, n, k, stride, pad)


def _convg_wgrad(*a):
    _wgrad('dis_convg_wgrad', *a)


def _convb_wgrad(*a):
    _wgrad('dis_convb_wgrad', *a)


def _act_bwd_f32(gy, y, act, gb):
    """Pre-activation gradient gpre = gy * act'(y) (dense fp32) of an nhwc gy; gy / y may be channel ranges of wider buffers (the
    gradient of a concatenation, an output written into one).  gb: where the bias gradient goes if one pass over gy can give both
    (None: not wanted).  -> (gpre, bias gradient written)"""
    n, h, w, c = gy.shape
    gpre = torch.empty(gy.shape, dtype=torch.float32, device=gy.device)
    ldy = _ld(y) if y is not None else 0
    if gb is not None and c <= 1024 and 256 % (c // 4) == 0 and gy.data_ptr() % 16 == 0 and (y is None or y.data_ptr() % 16 == 0):
        ws = torch.empty(lib.fn('dis_act_bwd_ld_bias_workspace')(c), dtype=torch.float32, device=gy.device)
        lib.call('dis_act_bwd_ld_bias', gy, _ld(gy), y, ldy, gpre, act, n * h * w, c, gb, ws)
        return gpre, True
    if gy.is_contiguous() and (y is None or y.is_contiguous()):
        lib.call('dis_act_bwd', gy, y, gpre, act, gy.numel())
    else:
        lib.call('dis_act_bwd_ld', gy, _ld(gy), y, ldy, gpre, act, n * h * w, c)
    return gpre, False


def _act_bwd_bf16(gy, y, act, gb):
    """_act_bwd_f32 on bf16 tensors (gpre bf16; the bias gradient is summed before gpre is rounded)"""
    n, h, w, c = gy.shape
    gpre = torch.empty(gy.shape, dtype=BF16, device=gy.device)
    ldy = _ld(y) if y is not None else 0
    if gb is not None and c <= 1024 and 256 % (c // 4) == 0:
        ws = torch.empty(lib.fn('dis_colsum_bf16_workspace')(c), dtype=torch.float32, device=gy.device)
        lib.call('dis_act_bwd_bf16_bias', gy, _ld(gy), y, ldy, gpre, act, n * h * w, c, gb, ws)
        return gpre, True
    lib.call('dis_act_bwd_bf16', gy, _ld(gy), y, ldy, gpre, act, n * h * w, c)
    return gpre, False


class _Storage(object):
    """What differs between the two activation storages: dtype and channel multiple (16-byte vectors) of the feature maps, the check
    of an input tensor, the forward-like launcher, the weight gradient, the entry points of the column sums and the channel copy (the
    bf16 one also takes its source's storage flag), and the pre-activation gradient."""

    def __init__(self, dtype, cmult, check, run, wgrad, colsum, copy, act_bwd):
        self.dtype, self.cmult, self.check, self.run, self.wgrad = dtype, cmult, check, run, wgrad
        self.colsum, self.copy, self.act_bwd = colsum, copy, act_bwd


_F32 = _Storage(torch.float32, 4, _chk_f32, _convg_run, _convg_wgrad, 'dis_colsum', 'dis_copy_channels', _act_bwd_f32)
_B16 = _Storage(BF16, 8, _chk_act, _convb_run, _convb_wgrad, 'dis_colsum_bf16', 'dis_copy_channels_bf16', _act_bwd_bf16)
_STORAGE = {torch.float32: _F32, BF16: _B16}


class _WriteChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, st, src, slot, zero_tail):
        buf, off, c = slot
        n, h, w, cs = src.shape
        assert cs == c and tuple(buf.shape[:3]) == (n, h, w)
        src = _nhwc(src)
        st.check(src)
        dst = buf[..., off:off + c]
        lib.call(st.copy, src, *((_isbf(src),) if st is _B16 else ()), _ld(src), dst, buf.shape[3], n * h * w, c,
                 buf.shape[3] - off - c if zero_tail else 0)
        ctx.src_dtype = src.dtype
        return dst

    @staticmethod
    def backward(ctx, g):
        return None, (g if g.dtype == ctx.src_dtype else g.float()), None, None   # (an fp32 source of a bf16 buffer)


def write_channels(src, slot, zero_tail=False):
    """copy the nhwc tensor src into a ConcatBuf slot; returns the slot's view (differentiable).  zero_tail: also zero the
    buffer's padding lanes behind the slot (the slot must be the concatenation's last part)."""
    return _WriteChannels.apply(_STORAGE[slot[0].dtype], src, slot, zero_tail)


def _colsum(G, c_real, out=None):
    """sum over all pixels of the first c_real channels of an nhwc tensor, fp32 or bf16 (into `out` if given)"""
    entry = _STORAGE[G.dtype].colsum
    npix = G.shape[0] * G.shape[1] * G.shape[2]
    if out is None:
        out = torch.empty(c_real, dtype=torch.float32, device=G.device)
    ws = torch.empty(lib.fn(entry + '_workspace')(c_real), dtype=torch.float32, device=G.device)
    lib.call(entry, G, _ld(G), 0, npix, c_real, out, ws)
    return out


def _conv_stream_shapes(st, x, weight, stride, pad, transposed, out_hw, out):
    """Shapes of a _ConvStream forward and its output y in the storage st: a new tensor, or the ConcatBuf slot `out` = (buffer, channel
    offset, channels).  -> (n, hin, win, cin_mem, cin_w, cout, k, hout, wout, y)"""
    n, hin, win, cin_mem = x.shape
    if transposed:
        cin_w, cout, k, _ = weight.shape
        hout, wout = out_hw
        if stride != 2 or hout > 2 * hin or wout > 2 * win:
            raise RuntimeError('transposed conv: stride 2 and out_hw <= 2x input expected')
    else:
        cout, cin_w, k, _ = weight.shape
        hout, wout = (hin + 2 * pad - k) // stride + 1, (win + 2 * pad - k) // stride + 1
    fp32 = st is _F32   # (bf16 storage: _chk_act has checked x; its buffers are told apart from fp32 ones by dtype)
    if (fp32 and cin_mem % 4) or cin_w > cin_mem or cout % st.cmult:
        raise RuntimeError(f'streaming conv: bad channel counts cin_mem={cin_mem} cin_w={cin_w} cout={cout}')
    if out is None:
        y = torch.empty((n, hout, wout, cout), dtype=st.dtype, device=x.device)
    else:
        buf, off, c = out
        if c != cout or tuple(buf.shape[:3]) != (n, hout, wout) or (not fp32 and buf.dtype != st.dtype):
            raise RuntimeError(f'streaming conv: out slot {tuple(buf.shape)}[{off}:{off + c}] does not fit ({n},{hout},{wout},{cout})')
        y = buf[..., off:off + c]
    return n, hin, win, cin_mem, cin_w, cout, k, hout, wout, y


class _ConvStream(torch.autograd.Function):
    """Conv2d / ConvTranspose2d(k,s2,p,op=1, cropped to out_hw) + bias + activation on nhwc tensors in the storage st.
    x (n,h,w,cin_mem): cin_mem % 4 == 0 and >= the weight's input channels (extra channels must be zero-weight padding lanes; their
    gradient is returned as zeros); in the bf16 storage x is bf16, or fp32 for the network input, and y is bf16."""

    @staticmethod
    def forward(ctx, st, x, weight, bias, stride, pad, act, transposed, out_hw, need_dgrad, out=None):
        x, weight = _nhwc(x), _c(weight)  # (x may be a channel range of a ConcatBuf)
        _chk(weight, bias)
        st.check(x)
        n, hin, win, cin_mem, cin_w, cout, k, hout, wout, y = _conv_stream_shapes(st, x, weight, stride, pad, transposed, out_hw, out)
        st.run(CONVG_TCONV if transposed else CONVG_CONV, x, weight, bias, y, n, hin, win, cin_mem, cin_w, hout, wout, cout, cout,
               k, stride, pad, act)
        ctx.save_for_backward(x, weight, y if act != ACT_NONE else None)
        ctx.bias_ref = bias  # (gradient sink lookup)
        ctx.cfg = (st, stride, pad, act, transposed, bias is not None, need_dgrad)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        st, stride, pad, act, transposed, has_bias, need_dgrad = ctx.cfg
        n, hin, win, cin_mem = x.shape
        gy = _nhwc(gy)
        _, hout, wout, cout = gy.shape
        k = weight.shape[2]
        cin_w = weight.shape[0] if transposed else weight.shape[1]
        want_gx = need_dgrad and ctx.needs_input_grad[1]
        # Shapes whose whole (tap, cin) x cout accumulator fits a workgroup's registers go through the one-pass fp32 kernels of
        # conv2d.hip: x and gy are read once instead of once per tap, and the bias gradient comes out of the same pass.  In the bf16
        # storage that is the network's first layer only: an fp32 x, no input gradient.
        onepass = (not transposed and x.is_contiguous() and x.dtype == torch.float32 and (st is _F32 or not want_gx)
                   and lib.fn('dis_conv2d_wgrad_workspace')(cin_mem, cout, k, stride) >= 0)
        gb, gb_ret = _sink_opt(ctx.bias_ref)
        gb_done = False
        if onepass and st is _B16:   # the one-pass kernel takes an fp32 pre-activation gradient
            gpre = torch.empty(gy.shape, dtype=torch.float32, device=gy.device)
            lib.call('dis_act_bwd_bf16_f32', gy, _ld(gy), y, _ld(y) if y is not None else 0, gpre, act, n * hout * wout, cout)
        elif act != ACT_NONE or not gy.is_contiguous():
            gpre, gb_done = st.act_bwd(gy, y, act, None if onepass else gb)
        else:
            gpre = gy
        gx = None
        if want_gx:
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            st.run(CONVG_TCONV_DGRAD if transposed else CONVG_CONV_DGRAD, gpre, weight, None, gx, n, hout, wout, cout, cout, hin, win,
                   cin_mem, cin_w, k, stride, pad, ACT_NONE)
        gw, gw_ret = _sink(weight)
        if onepass:
            ws = torch.empty(lib.fn('dis_conv2d_wgrad_workspace')(cin_mem, cout, k, stride), dtype=torch.float32, device=x.device)
            _conv_wgrad_any(x, gpre, gw, gb, ws, n, hin, win, cin_mem, cin_w, cout, k, stride, pad)
        else:
            if transposed:
                st.wgrad(gpre, hout, wout, cout, cout, x, hin, win, cin_mem, cin_w, gw, n, k, stride, pad)
            else:
                st.wgrad(x, hin, win, cin_mem, cin_w, gpre, hout, wout, cout, cout, gw, n, k, stride, pad)
            if has_bias and not gb_done:
                _colsum(gpre, cout, out=gb)
        _sinks_written()
        return None, gx, gw_ret, gb_ret, None, None, None, None, None, None, None


def convg(x, weight, bias, stride=1, pad=0, act=ACT_NONE, need_dgrad=True, out=None, dtype=torch.float32):
    """Conv2d on an nhwc tensor through the streaming MFMA kernel (any channel count that is a multiple of 4).
    out: optional ConcatBuf.slot the result is written into (the returned tensor is that channel range).
    dtype=torch.bfloat16: bf16 activation storage (the result is bf16; x bf16, or fp32 for the network input)."""
    return _ConvStream.apply(_STORAGE[dtype], x, weight, bias, stride, pad, act, False, None, need_dgrad, out)


def convg_transposed(x, weight, bias, out_hw, pad=1, act=ACT_NONE, out=None, dtype=torch.float32):
    """ConvTranspose2d(k=3, stride=2, padding=pad, output_padding=1) cropped to out_hw (crop_like)."""
    return _ConvStream.apply(_STORAGE[dtype], x, weight, bias, 2, pad, act, True, tuple(out_hw), True, out)


def _head_stream_fwd(ctx, st, x, weight, bias, alpha, offset):
    """A disparity head as a one-channel streaming conv + alpha*sigmoid(. - offset); y is float32"""
    n, h, w, cin = x.shape
    k = weight.shape[2]
    y = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device)
    st.run(CONVG_CONV, x, weight, bias, y.view(n, h, w, 1), n, h, w, cin, weight.shape[1], h, w, 1, 1, k, 1, k // 2, ACT_NONE)
    lib.call('dis_sigmoid_affine_fwd', y, y, float(alpha), float(offset), y.numel())
    ctx.save_for_backward(x, weight, y)
    ctx.alpha = float(alpha)
    ctx.bias_ref = bias
    return y


def _head_stream_bwd(ctx, st, gy):
    x, weight, y = ctx.saved_tensors
    n, h, w, cin = x.shape
    k = weight.shape[2]
    cin_w = weight.shape[1]
    gpre4 = torch.empty((n, h, w, 4), dtype=torch.float32, device=x.device)
    lib.call('dis_sigmoid_affine_bwd', y, _c(gy), gpre4, ctx.alpha, n * h * w)
    gx = torch.empty_like(x)
    st.run(CONVG_CONV_DGRAD, gpre4, weight, None, gx, n, h, w, 4, 1, h, w, cin, cin_w, k, 1, k // 2, ACT_NONE)
    gw, gw_ret = _sink(weight)
    gb, gb_ret = _sink(ctx.bias_ref)
    st.wgrad(x, h, w, cin, cin_w, gpre4, h, w, 4, 1, gw, n, k, 1, k // 2)
    _colsum(gpre4, 1, out=gb)
    _sinks_written()
    return None, gx, gw_ret, gb_ret, None, None


class _HeadStream(torch.autograd.Function):
    """Conv2d(cin,1,3,pad 1) + alpha*sigmoid(. - offset): x nhwc in the storage st (fp32: any cin % 4 == 0) -> y planar (n,1,h,w),
    float32."""

    @staticmethod
    def forward(ctx, st, x, weight, bias, alpha, offset):
        x, weight, bias = _c(x), _c(weight), _c(bias)
        _chk(weight, bias)
        st.check(x)
        n, h, w, cin = x.shape
        ctx.st = st
        # the one-pass head kernels (fp32 x, 16 / 32 channels)
        ctx.direct = st is _F32 and weight.shape[2] == 3 and cin in (16, 32) and weight.shape[1] == cin
        if ctx.direct:
            y = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device)
            lib.call('dis_disp_head_fwd', x, weight, bias, y, n, h, w, cin, float(alpha), float(offset))
            ctx.save_for_backward(x, weight, y)
            ctx.alpha = float(alpha)
            ctx.bias_ref = bias
            return y
        return _head_stream_fwd(ctx, st, x, weight, bias, alpha, offset)

    @staticmethod
    def backward(ctx, gy):
        if not ctx.direct:
            return _head_stream_bwd(ctx, ctx.st, gy)
        x, weight, y = ctx.saved_tensors
        n, h, w, cin = x.shape
        gw, gw_ret = _sink(weight)
        gb, gb_ret = _sink(ctx.bias_ref)
        gx = torch.empty_like(x)
        ws = torch.empty(lib.fn('dis_disp_head_bwd_workspace')(n, h, w, cin), dtype=torch.float32, device=x.device)
        lib.call('dis_disp_head_bwd', x, weight, y, _c(gy), gx, gw, gb, ws, n, h, w, cin, ctx.alpha)
        _sinks_written()
        return None, gx, gw_ret, gb_ret, None, None


def disp_head_g(x, weight, bias, alpha, offset=3.0):
    return _HeadStream.apply(_STORAGE[x.dtype], x, weight, bias, alpha, offset)


# --------------------------------------------------------------------------------------------------
# GroupNorm(1 group) (+ residual + activation)
# --------------------------------------------------------------------------------------------------
class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stats, gamma, beta, residual, act, eps, in_act=ACT_NONE, join=None, x_lazy=False, defer=False):
        ctx.x_lazy = x_lazy   # the producer of x redeems a token for the elementwise backward pass (_GN_LAZY)
        x = _c(x)
        residual = _c(residual) if residual is not None else None
        _chk(x, gamma, beta, residual)
        n = x.shape[0]
        c = x.shape[-1]
        hw = x.numel() // (n * c)
        if stats is None:
            stats = _zeros_d(2 * n, x.device)
            lib.call('dis_gn_stats', x, stats, n, hw * c)
        y = torch.empty_like(x)
        if not defer:   # (defer: the 3x3 conv that consumes y first writes it, see _GN_PENDING)
            lib.call('dis_gn_apply', x, stats, gamma, beta, residual, y, n, hw, c, act, float(eps))
        ctx.save_for_backward(x, stats, gamma, y if act != ACT_NONE else None)
        ctx.cfg = (n, hw, c, act, float(eps), residual is not None, in_act)
        ctx.beta_ref = beta
        ctx.join = join
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, gamma, y = ctx.saved_tensors
        n, hw, c, act, eps, has_res, in_act = ctx.cfg
        gy = _c(gy)
        gg, gg_ret = _sink(gamma)
        gb, gb_ret = _sink(ctx.beta_ref)
        pre = _GN_PRE.pop(gy.data_ptr(), None)
        if pre is not None and ((not has_res and act == ACT_NONE) or (has_res and act == ACT_SELU and in_act == ACT_NONE)):
            # the consumer whose backward ran second left the sums of the complete g: a plain GroupNorm output with two consumers,
            # or (residual + SELU) gy already IS the gradient wrt the pre-activation value (the producing input-gradient launch
            # multiplied by SELU'(y)), which doubles as the residual gradient, and one elementwise pass gives gx
            gx = _gn_bwd_from_sums(gy, x, stats, gamma, pre[0], pre[1], gg, gb, eps, in_act, ctx.x_lazy)
            gres = gy.view(x.shape) if has_res else None
        elif pre is not None:
            # the producer has ALREADY turned gy into the pre-activation gradient and formed its channel sums: the generic
            # two-pass form below would apply act' a second time.  No networks here reach this; a new caller must not do so silently.
            raise RuntimeError(f'group_norm backward: channel sums were registered for this gradient but no from-sums form matches '
                               f'(residual={has_res}, act={act}, in_act={in_act})')
        elif (ctx.x_lazy and GN_LAZY and GN_RES_SUMS and c in (16, 32) and x.dim() == 4 and (act == ACT_NONE or has_res) and
                (in_act == ACT_NONE or act == ACT_NONE) and lib.fn('dis_get_conv_split')() == 1):
            # nobody left channel sums for this gradient (it comes from a join, a resize, a feature warp), but the producer of x
            # redeems tokens: ONE pass forms g = gy act'(y) (the residual gradient, stored), and the sums of g and g x; the
            # elementwise pass rides on the producer's input-gradient launch (instead of a reduce and an apply launch over gy, y, x)
            ab, slots = _gn_sums(n, c, x.device)
            gres = torch.empty_like(x) if (has_res or act != ACT_NONE) else None
            lib.call('dis_gn_bwd_res_sums', gy, y, x, gres, ab, slots, n, hw, c, act)
            g_ = gres if gres is not None else gy.view(x.shape)
            gx = _gn_lazy_defer(g_, x, stats, gamma, ab, slots, gg, gb, n, hw, c, eps, in_act, uid=ctx.x_lazy)
            if not has_res:
                gres = None
        else:
            gres = torch.empty_like(x) if has_res else None
            gx = _gn_apply_bwd(gy, y, x, stats, gamma, gres, gg, gb, act, eps, in_act)
        if gres is not None and ctx.join is not None:
            if ctx.join.buf is None:
                gres = ctx.join.first(gres)
            else:  # the other consumer ran first (not the case in the networks here): plain accumulation
                gres = ctx.join.take(gres.shape).add_(gres)
        _sinks_written()
        return gx, None, gg_ret, gb_ret, gres, None, None, None, None, None, None


def c_ok(x):
    return x.shape[-1] in (16, 32)


GN_DEFER = _os.environ.get('DIS_GN_DEFER', '1') != '0'
GN_RES_SUMS = _os.environ.get('DIS_GN_RES_SUMS', '1') != '0'   # =0: dis_gn_apply_bwd (reduce + apply launches) where no conv left the channel sums


def group_norm(x, gamma, beta, stats=None, residual=None, act=ACT_NONE, eps=1e-5, in_act=ACT_NONE, join=None, defer=False):
    """GroupNorm(1 group) over all but the first dim of an nhwc tensor; y = act(gn(x) (+ residual)).
    in_act: x is the output of that activation (conv2d(..., act, gy_is_pre=True)); the backward then returns the
    gradient wrt the producer's pre-activation output.
    defer (residual + SELU form with known statistics only): y is NOT written here; the caller guarantees that its first reader is
    conv2d(y, ...) - which forms the values on load and stores them - or calls ops.realize(y) (see _GN_PENDING)."""
    defer = bool(defer and GN_DEFER and residual is not None and act == ACT_SELU and in_act == ACT_NONE and stats is not None and
                 x.dim() == 4 and c_ok(x) and BF16X3)
    y = _GroupNorm.apply(x, stats, gamma, beta, residual, act, eps, in_act, join, int(getattr(x, '_gn_lazy_ok', 0)), defer)
    if defer:
        y._pending_gn = (_c(x), stats, gamma, beta, _c(residual), float(eps))
        _GN_PENDING[y.data_ptr()] = True
    if residual is not None and act == ACT_SELU and in_act == ACT_NONE:
        y._gn_res_src = (x,)   # (a ResNetBlock that takes y as its input hands this to its first conv: conv2d(gnres=...))
    elif residual is None and act == ACT_NONE and c_ok(x):
        y._gn_plain_src = (x, None)   # (two-consumer form: Block2D3D hands it to the consumer whose backward runs second)
    return y


# --------------------------------------------------------------------------------------------------
# multi-frame: gathered/warped features, geometry, slot weighting, Conv3D
# --------------------------------------------------------------------------------------------------
# DIS_GATHER_GNRES=0: the feature warp's backward leaves the plain gradient and the GroupNorm behind it runs dis_gn_bwd_res_sums (A/B)
GATHER_GNRES = _os_env.environ.get('DIS_GATHER_GNRES', '1') != '0'


class _GatherWarpedFeat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, flows, csr, join, gnres=None):
        feat, flows = _c(feat), _c(flows)
        _chk(feat, flows)
        tl, bs, h, w, c = feat.shape
        assert flows.shape == (tl * tl, bs, h, w, 2), flows.shape
        out = torch.empty((tl, bs, h, w, tl, c), dtype=torch.float32, device=feat.device)
        lib.call('dis_gather_warped_feat_fwd', feat, flows, out, tl, bs, h, w, c)
        # gnres = (x2,): feat IS y = SELU(GroupNorm(x2) + residual) and the other consumer of y shares `join`: the backward pass that
        # runs second completes the gradient wrt y - if that is this one, it also does the GroupNorm backward's first pass (below)
        ctx.gnres = bool(gnres is not None and join is not None and csr is not None and GATHER_GNRES and GN_RES_SUMS and GN_LAZY and
                         2 * c <= 64 and tuple(gnres[0].shape[-3:]) == (h, w, c) and gnres[0].numel() == feat.numel())
        if ctx.gnres:
            ctx.save_for_backward(flows, csr, feat, _c(gnres[0]))
        else:
            ctx.save_for_backward(flows, csr)
        ctx.shape = feat.shape
        ctx.join = join
        return out

    @staticmethod
    def backward(ctx, g):
        flows, csr = ctx.saved_tensors[:2]
        tl, bs, h, w, c = ctx.shape
        join = ctx.join
        second = join is not None and join.buf is not None
        if csr is not None:
            init = join.take(ctx.shape) if second else None
            gf = init if second else torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
            done = False
            if ctx.gnres and second and lib.fn('dis_get_conv_split')() == 1:
                # this launch completes the gradient wrt y = SELU(GroupNorm(x2) + residual): it stores g SELU'(y) and leaves the channel
                # sums of the GroupNorm's backward (_GroupNorm.backward finds them: no pass over g, y, x2 of its own)
                y, x2 = ctx.saved_tensors[2:4]
                ab, slots = _gn_sums(tl * bs, c, g.device)
                if lib.call_try('dis_gather_warped_feat_bwd_csr_gnres', _c(g), csr, init, gf, y, x2, ab, slots, ACT_SELU, tl, bs, h, w, c):
                    _GN_PRE[gf.data_ptr()] = (ab, slots)
                    done = True
            if not done:
                lib.call('dis_gather_warped_feat_bwd_csr', _c(g), csr, init, gf, tl, bs, h, w, c)
        else:
            gf = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
            lib.call('dis_gather_warped_feat_bwd', _c(g), flows, gf, tl, bs, h, w, c)
            if second:
                gf.add_(join.take(ctx.shape))
        if join is not None and not second:
            gf = join.first(gf)
        return gf, None, None, None, None


def gather_csr(flows):
    """Scatter index of gather_warped_feat for `flows` (tl*tl,bs,h,w,2): build once per step and pass to every
    gather_warped_feat call that uses these flows; the backward then runs without atomics (deterministic)."""
    flows = _c(flows)
    _chk(flows)
    t2, bs, h, w, _ = flows.shape
    tl = int(round(t2 ** 0.5))
    n = lib.fn('dis_gather_csr_workspace')(tl, bs, h, w)
    if n < 0:
        raise lib.DisHipError('gather_csr: unsupported shape')
    csr = torch.empty(n, dtype=torch.int32, device=flows.device)
    lib.call('dis_gather_csr_build', flows, csr, tl, bs, h, w)
    return csr


def gather_warped_feat(feat, flows, csr=None, join=None, gnres=None):
    """gnres = (x2,): feat is SELU(GroupNorm(x2) + residual) (group_norm's `_gn_res_src`) whose other consumer shares `join`"""
    return _GatherWarpedFeat.apply(feat, flows, csr, join, gnres)


def mf_geometry(depth_core, R, t, flows_core, Kinv, u_step, v_step):
    depth_core, R, t, flows_core = _c(depth_core), _c(R), _c(t), _c(flows_core)
    _chk(depth_core, R, t, flows_core)
    tl, bs, h, w = depth_core.shape
    out = torch.empty((tl, bs, h, w, tl, 4), dtype=torch.float32, device=depth_core.device)
    lib.call('dis_mf_geometry', depth_core, R, t, flows_core, Kinv, int(u_step), int(v_step), out, tl, bs, h, w)
    return out


def mf_geometry_resize(geom, size):
    tl, bs, hin, win, _, _ = geom.shape
    out = torch.empty((tl, bs, size[0], size[1], tl, 4), dtype=torch.float32, device=geom.device)
    lib.call('dis_mf_geometry_resize', geom, out, tl, bs, hin, win, size[0], size[1])
    return out


class _MaskWeightSlots(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wf, geom, join):
        wf, geom = _c(wf), _c(geom)
        tl, bs, h, w, s, c = wf.shape
        out = torch.empty_like(wf)
        lib.call('dis_mask_weight_slots', wf, geom, out, tl * bs * h * w, s, c, 0)
        ctx.save_for_backward(geom)
        ctx.join = join
        return out

    @staticmethod
    def backward(ctx, g):
        (geom,) = ctx.saved_tensors
        g = _c(g)
        tl, bs, h, w, s, c = g.shape
        join = ctx.join or _SOLE
        out, second = join.target(g)
        lib.call('dis_mask_weight_slots', g, geom, out, tl * bs * h * w, s, c, 1 if second else 0)
        return join.result(out, second), None, None


def mask_weight_slots(wf, geom, join=None):
    return _MaskWeightSlots.apply(wf, geom, join)


def conv3d_select(geom, stride):
    """top-9 neighbour ids per output pixel (tl,bs,ho,wo,9) uint8; depends on the geometry only."""
    geom = _c(geom)
    _chk(geom)
    tl, bs, h, wd, s, _ = geom.shape
    ho = (h + 2 - 3) // stride + 1
    wo = (wd + 2 - 3) // stride + 1
    idx = torch.empty((tl, bs, ho, wo, 9), dtype=torch.uint8, device=geom.device)
    lib.call('dis_conv3d_knn_select', geom, idx, tl, bs, h, wd, stride)
    return idx


class _Conv3dKnn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, geom, wf, d1w, d1b, d2w, d2b, w, idx, stride, join=None):
        geom, wf = _c(geom), _c(wf)
        d1w, d1b, d2w, d2b, w = [_c(p) for p in (d1w, d1b, d2w, d2b, w)]
        _chk(geom, wf, d1w, d1b, d2w, d2b, w)
        tl, bs, h, wd, s, c = wf.shape
        assert c == 32 and s == tl
        ho = (h + 2 - 3) // stride + 1
        wo = (wd + 2 - 3) // stride + 1
        assert idx.dtype == torch.uint8 and tuple(idx.shape) == (tl, bs, ho, wo, 9) and idx.is_contiguous()
        y = torch.empty((tl, bs, ho, wo, c), dtype=torch.float32, device=wf.device)
        agg = torch.empty_like(y) if any(ctx.needs_input_grad) else None   # (the backward reads the aggregate back)
        lib.call('dis_conv3d_knn_fwd_agg', geom, wf, d1w, d1b, d2w, d2b, w, idx, y, agg, tl, bs, h, wd, stride)
        ctx.save_for_backward(geom, wf, d1w, d1b, d2w, d2b, w, idx, y, agg)
        ctx.stride = stride
        ctx.join = join
        return y

    @staticmethod
    def backward(ctx, gy):
        geom, wf, d1w, d1b, d2w, d2b, w, idx, y, agg = ctx.saved_tensors
        tl, bs, h, wd, s, c = wf.shape
        join = ctx.join or _SOLE
        sunk = _sink_block((w, d1w, d1b, d2w, d2b))  # the kernel's parameter-gradient block IS the flat buffer's order
        gp = sunk if sunk is not None else torch.empty(1632, dtype=torch.float32, device=wf.device)
        # class-ordered read-modify-write of the feature-gradient rows: ADDS to the rows
        gwf, second = join.target(wf, torch.zeros_like)
        acc = torch.empty(lib.fn('dis_conv3d_knn_bwd_det_workspace')(tl, bs, h, wd, ctx.stride), dtype=torch.float32,
                          device=wf.device)
        lib.call('dis_conv3d_knn_bwd_det', geom, wf, d1w, d1b, d2w, d2b, w, idx, y, agg, _c(gy), gwf, gp, acc, tl, bs, h, wd,
                 ctx.stride)
        gwf = join.result(gwf, second)
        _sinks_written()
        if sunk is not None:
            return (None, gwf, None, None, None, None, None, None, None, None)
        return (None, gwf, gp[1024:1072].view(16, 3), gp[1072:1088], gp[1088:1600].view(32, 16), gp[1600:1632],
                gp[0:1024].view(32, 32), None, None, None)


def conv3d_knn(geom, wf, d1w, d1b, d2w, d2b, w, idx, stride, join=None):
    """y (tl,bs,ho,wo,32) = SELU(agg @ w) for the neighbour sets `idx` (from conv3d_select)."""
    return _Conv3dKnn.apply(geom, wf, d1w, d1b, d2w, d2b, w, idx, stride, join)


# --------------------------------------------------------------------------------------------------
# optimiser
# --------------------------------------------------------------------------------------------------
def adam_step_dev(param, grad, exp_avg, exp_avg_sq, state, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """Adam with the step counter / bias corrections in the 4 x int32 device tensor `state` (advanced by the call):
    safe to capture in a hipGraph."""
    _chk(param, grad, exp_avg, exp_avg_sq)
    if not state.is_cuda or state.dtype != torch.int32 or state.numel() < 4:
        raise RuntimeError('adam_step_dev: state must be a 4-element int32 CUDA(HIP) tensor')
    lib.call('dis_adam_step_dev', param, grad, exp_avg, exp_avg_sq, param.numel(), float(lr), float(beta1), float(beta2),
             float(eps), state, float(grad_scale))
    params_changed()   # what this step's batch launch packed is stale (inference before the next step packs per call)


def adam_step_hyper(param, grad, exp_avg, exp_avg_sq, state, hyper, stats=None, partials=None, mode=0, beta1=0.9,
                    beta2=0.999, eps=1e-8, grad_scale=1.0):
    """adam_step_dev with the learning rate (hyper[0]) and max_norm (hyper[1]) read from the 4-float device tensor `hyper`, and,
    with mode bit 0 / bit 1, clip-by-global-norm / skip-on-a-non-finite-norm decided on the device (`stats`: 4 doubles {norm,
    coefficient, skipped steps, skipped this call}; `partials`: dis_adam_step_hyper_workspace doubles).  Safe to capture."""
    _chk(param, grad, exp_avg, exp_avg_sq)
    if not state.is_cuda or state.dtype != torch.int32 or state.numel() < 4:
        raise RuntimeError('adam_step_hyper: state must be a 4-element int32 CUDA(HIP) tensor')
    if not hyper.is_cuda or hyper.dtype != torch.float32 or hyper.numel() < 4:
        raise RuntimeError('adam_step_hyper: hyper must be a 4-element float32 CUDA(HIP) tensor')
    if mode != 0:
        if stats is None or not stats.is_cuda or stats.dtype != torch.float64 or stats.numel() < 4:
            raise RuntimeError('adam_step_hyper: stats must be a 4-element float64 CUDA(HIP) tensor')
        need = lib.fn('dis_adam_step_hyper_workspace')(param.numel())
        if partials is None or not partials.is_cuda or partials.dtype != torch.float64 or need < 0 or partials.numel() < need:
            raise RuntimeError(f'adam_step_hyper: partials must be a float64 CUDA(HIP) tensor of {need} elements')
    lib.call('dis_adam_step_hyper', param, grad, exp_avg, exp_avg_sq, param.numel(), hyper, float(beta1), float(beta2),
             float(eps), state, stats, partials, int(mode), float(grad_scale))
    params_changed()   # (as adam_step_dev)


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _chk(param, grad, exp_avg, exp_avg_sq)
    params_changed()
    lib.call('dis_adam_step', param, grad, exp_avg, exp_avg_sq, param.numel(), float(lr), float(beta1), float(beta2),
             float(eps), int(step), float(grad_scale))


# ----------------------------------------------------------------------------------------------------------------------
# batch assembly for packed track files (data/packed.py)
# ----------------------------------------------------------------------------------------------------------------------
# DisTrackOut field -> (batch key, trailing shape after (tl, bs)); flow: (tl * tl, bs, 2, h, w)
_TRACK_KEYS = {'im': 'im0', 'ambient': 'ambient0', 'disp': 'disp0', 'sgm_disp': 'sgm_disp', 'primary_disp': 'primary_disp',
               'pseudo_gt': 'pseudo_gt', 'flow': '_flow_stacked', 'R': 'R', 't': 't'}


def assemble_tracks(raw, perm, bs, tl, h, w, has_sgm=False, primary=False, pseudo=False, want_sgm=None, flows=True,
                    record_stride=None, out=None):
    """dis_assemble_tracks: `bs` packed records (data.packed.record_layout(h, w, has_sgm, primary, pseudo); record b at
    raw[b * record_stride:], default stride: the record size) and the (bs, tl) int32 frame orders `perm` -> the step's inputs in
    their final layout, one launch on the current stream: im0 / ambient0 / disp0 [/ sgm_disp / primary_disp / pseudo_gt]
    (tl, bs, 1, h, w), R (tl, bs, 3, 3), t (tl, bs, 3), _flow_stacked (tl * tl, bs, 2, h, w) with zero i == j planes.
    want_sgm: deliver sgm_disp (default: when the records have it); flows=False: no _flow_stacked.  out: a dict holding
    tensors of exactly these shapes to write into (the static buffers of a captured step); default: fresh tensors.  Returns a
    data.packed.AssembledBatch (a dict that Worker.copy_data takes as it is)."""
    from .data import packed as _packed
    lay = _packed.record_layout(h, w, has_sgm, primary, pseudo)
    stride = lay['size'] if record_stride is None else int(record_stride)
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.float32 and raw.dim() == 1 and raw.is_contiguous()):
        raise RuntimeError('assemble_tracks: raw must be a contiguous 1-D float32 CUDA(HIP) tensor: the HIP path is the only path')
    if not (perm.is_cuda and perm.dtype == torch.int32 and perm.is_contiguous() and tuple(perm.shape) == (bs, tl)):
        raise RuntimeError(f'assemble_tracks: perm must be a contiguous int32 CUDA(HIP) tensor of shape ({bs}, {tl})')
    if bs > 0 and stride > 0 and raw.numel() < (bs - 1) * stride + lay['size']:
        raise RuntimeError(f'assemble_tracks: raw holds {raw.numel()} floats, {bs} records of stride {stride} need '
                           f'{(bs - 1) * stride + lay["size"]}')
    want = {'im': True, 'ambient': True, 'disp': True, 'R': True, 't': True, 'flow': bool(flows), 'primary_disp': bool(primary),
            'pseudo_gt': bool(pseudo), 'sgm_disp': bool(has_sgm) if want_sgm is None else bool(want_sgm)}
    shapes = {'R': (tl, bs, 3, 3), 't': (tl, bs, 3), 'flow': (tl * tl, bs, 2, h, w)}
    L, O = lib.TrackLayout(), lib.TrackOut()
    res = _packed.AssembledBatch()
    for f in lib.TRACK_FIELDS:
        setattr(L, f, lay.get(f, -1))
        if not want[f]:
            continue
        shape = shapes.get(f, (tl, bs, 1, h, w))
        if out is None:
            t = torch.empty(shape, dtype=torch.float32, device=raw.device)
        else:
            t = out[_TRACK_KEYS[f]]
            _chk(t)
            if tuple(t.shape) != shape or t.device != raw.device:
                raise RuntimeError(f'assemble_tracks: out[{_TRACK_KEYS[f]!r}] is {tuple(t.shape)} on {t.device}, expected {shape} '
                                   f'on {raw.device}')
        setattr(O, f, t.data_ptr())
        res[_TRACK_KEYS[f]] = t
    lib.call('dis_assemble_tracks', raw, stride, perm, _ct.addressof(L), _ct.addressof(O), int(bs), int(tl), int(h), int(w))
    return res


# ----------------------------------------------------------------------------------------------------------------------
# track rendering (csrc/render.hip; data/render.py samples the scenes and writes the tracks)
# ----------------------------------------------------------------------------------------------------------------------
def render_track(verts, faces, albedo, R, t, K, baseline, blend, pattern, want_ids=True, workspace=None):
    """dis_render_track: the triangle mesh verts (nv, 3) float32 / faces (nf, 3) int32 / albedo (nf) float32 seen by the tl <= 4 cameras
    R (tl, 3, 3), t (tl, 3) (X_c = R X_w + t) with intrinsics K (3 x 3, host: numpy or a CPU tensor), a rectified projector at
    +baseline and the (h, w) pattern -> a dict of device tensors: im, ambient, disp (tl, 1, h, w), flow (tl * tl, 2, h, w) (entry
    i * tl + j = flow_ij, zero diagonal) and, with want_ids, tri_id (tl, h, w) int32 (-1: no triangle) and lit (tl, h, w).  Image
    formation: include/dis_hip.h, section "track rendering".  Two launches on the current stream; workspace: an optional uint8 tensor
    of at least dis_render_workspace(...) bytes to reuse between calls."""
    _chk(verts, albedo, R, t, pattern)
    if not (faces.is_cuda and faces.dtype == torch.int32 and faces.is_contiguous()):
        raise RuntimeError('render_track: faces must be a contiguous int32 CUDA(HIP) tensor: the HIP path is the only path')
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or albedo.numel() != faces.shape[0]:
        raise RuntimeError('render_track: verts (nv, 3), faces (nf, 3) and albedo (nf) are expected')
    tl = int(R.shape[0])
    if tuple(R.shape) != (tl, 3, 3) or tuple(t.shape) != (tl, 3) or pattern.dim() != 2:
        raise RuntimeError('render_track: R (tl, 3, 3), t (tl, 3) and a pattern (h, w) are expected')
    h, w = int(pattern.shape[0]), int(pattern.shape[1])
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    need = lib.fn('dis_render_workspace')(nv, nf, tl, h, w)
    if need < 0:
        raise lib.DisHipError(f'dis_render_workspace: unsupported extents nv={nv} nf={nf} tl={tl} h={h} w={w}')
    dev = verts.device
    workspace = _workspace('render_track', need, workspace, dev)
    res = {'im': torch.empty((tl, 1, h, w), dtype=torch.float32, device=dev),
           'ambient': torch.empty((tl, 1, h, w), dtype=torch.float32, device=dev),
           'disp': torch.empty((tl, 1, h, w), dtype=torch.float32, device=dev),
           'flow': torch.empty((tl * tl, 2, h, w), dtype=torch.float32, device=dev)}
    if want_ids:
        res['tri_id'] = torch.empty((tl, h, w), dtype=torch.int32, device=dev)
        res['lit'] = torch.empty((tl, h, w), dtype=torch.float32, device=dev)
    O = _out_struct(lib.RenderOut, res)
    lib.call('dis_render_track', verts, faces, albedo, nv, nf, R, t, lib.host_floats(_k4(K)), float(baseline), float(blend), pattern,
             _ct.addressof(O), tl, h, w, workspace)
    return res


def sgm_disparity(im, pattern, ndisp=64, p1=7, p2=60, uniq=5, lr=1, want_debug=False, workspace=None):
    """dis_sgm_disparity: 9 x 7 census + 8-path semi-global matching of the IR frames im (n, 1, H, W) or (n, H, W) against the projector
    pattern (H, W) -> disp with the shape of im, 0 where the match is invalid (include/dis_hip.h, section "semi-global matching";
    tests/sgm_ref.py restates it in numpy and the kernels equal it bit for bit).  ndisp: 64, 128 or 256 candidates; 0 < p1 < p2 <= 127;
    uniq in [0, 100) per cent; lr >= 0 pixels.  want_debug: also a dict with d_int (n, H, W) int32 (the winning candidate of every pixel,
    valid or not), vol (n, H, W, ndisp) int16 (the aggregated cost) and census (n + 1, H, W) int64 (the pattern's last).  The inputs are
    data: no autograd.  Ten launches on the current stream; workspace: an optional uint8 tensor of at least dis_sgm_workspace(...)
    bytes to reuse between calls (and what makes the call capturable without an allocation)."""
    _chk(im, pattern)
    if not ((im.dim() == 3 or (im.dim() == 4 and im.shape[1] == 1)) and pattern.dim() == 2 and tuple(im.shape[-2:]) == tuple(pattern.shape)):
        raise RuntimeError('sgm_disparity: im (n, 1, H, W) or (n, H, W) and a pattern (H, W) are expected')
    n, h, w = int(im.shape[0]), int(im.shape[-2]), int(im.shape[-1])
    ndisp, p1, p2, uniq, lr = int(ndisp), int(p1), int(p2), int(uniq), int(lr)
    need = lib.fn('dis_sgm_workspace')(n, h, w, ndisp)
    if need < 0:
        raise lib.DisHipError(f'dis_sgm_workspace: unsupported extents n={n} h={h} w={w} ndisp={ndisp}')
    if not (0 < p1 < p2 <= 127 and 0 <= uniq < 100 and lr >= 0):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'sgm_disparity: unsupported configuration p1={p1} p2={p2} uniq={uniq} lr={lr}')
    dev = im.device
    workspace = _workspace('sgm_disparity', need, workspace, dev)
    disp = torch.empty_like(im)
    dbg = None
    if want_debug:
        dbg = {'d_int': torch.empty((n, h, w), dtype=torch.int32, device=dev),
               'vol': torch.empty((n, h, w, ndisp), dtype=torch.int16, device=dev),
               'census': torch.empty((n + 1, h, w), dtype=torch.int64, device=dev)}
    lib.call('dis_sgm_disparity', im, pattern, disp, dbg and dbg['d_int'], dbg and dbg['vol'], dbg and dbg['census'], n, h, w, ndisp,
             p1, p2, uniq, lr, workspace)
    return (disp, dbg) if want_debug else disp


def speckle_filter(disp, max_size=100, max_diff=1.0, want_debug=False, workspace=None):
    """dis_speckle_filter: the disparity maps disp (n, 1, H, W) or (n, H, W) with every 4-connected component of similar disparity of at
    most max_size pixels set to 0 -> a new tensor with the shape of disp (include/dis_hip.h, section "speckle filter"; tests/speckle_ref.py
    restates it in numpy and the kernels equal it bit for bit).  Valid pixels are 0 < d < inf; neighbours are linked when both are valid
    and |d_p - d_q| <= max_diff in fp32; max_size >= 0 (0 keeps every valid pixel), max_diff >= 0 and finite.  want_debug: also a dict
    with label (n, H, W) int32 (y W + x of the component's first pixel, -1: invalid) and size (n, H, W) int32 (its pixel count, 0: invalid).
    The input is data: no autograd.  Four launches on the current stream; workspace: an optional uint8 tensor of at least
    dis_speckle_workspace(...) bytes to reuse between calls (and what makes the call capturable without an allocation)."""
    _chk(disp)
    if not (disp.dim() == 3 or (disp.dim() == 4 and disp.shape[1] == 1)):
        raise RuntimeError('speckle_filter: disp (n, 1, H, W) or (n, H, W) is expected')
    n, h, w = int(disp.shape[0]), int(disp.shape[-2]), int(disp.shape[-1])
    max_size, max_diff = int(max_size), float(max_diff)
    need = lib.fn('dis_speckle_workspace')(n, h, w)
    if need < 0:
        raise lib.DisHipError(f'dis_speckle_workspace: unsupported extents n={n} h={h} w={w}')
    if not (0 <= max_size <= 0x7fffffff and 0 <= max_diff <= 3.4028234663852886e38):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'speckle_filter: unsupported configuration max_size={max_size} max_diff={max_diff}')
    dev = disp.device
    workspace = _workspace('speckle_filter', need, workspace, dev)
    out = torch.empty_like(disp)
    dbg = None
    if want_debug:
        dbg = {'label': torch.empty((n, h, w), dtype=torch.int32, device=dev),
               'size': torch.empty((n, h, w), dtype=torch.int32, device=dev)}
    lib.call('dis_speckle_filter', disp, out, dbg and dbg['label'], dbg and dbg['size'], n, h, w, max_size, max_diff, workspace)
    return (out, dbg) if want_debug else out


def disp_densify(disp, max_gap=16, min_dirs=6, max_spread=2.0, median=1, want_state=False, workspace=None):
    """dis_disp_densify: the disparity maps disp (n, 1, H, W) or (n, H, W) with the holes inside one surface filled and a median over the
    valid pixels -> a new tensor with the shape of disp (include/dis_hip.h, section "disparity densification"; tests/densify_ref.py
    restates it in numpy and the kernels equal it bit for bit).  Valid pixels are 0 < d < inf and every other element comes out as
    +0.0.  Fill (max_gap 1 .. 32, 0: off): an invalid pixel takes the lower median of the first valid pixels met within max_gap steps in
    the 8 directions when at least min_dirs (1 .. 8) of them meet one and the largest and the smallest differ by at most max_spread
    (in [0, FLT_MAX]).  Median (1 or 2, 0: off): every valid pixel becomes the lower median of the valid pixels of its (2 r + 1)^2
    window.  want_state: also state (n, H, W) uint8 - 0 invalid, 1 valid in the input, 2 filled.  The input is data: no autograd.
    At most two launches on the current stream; workspace: an optional uint8 tensor of at least dis_disp_densify_workspace(...) bytes
    to reuse between calls (and what makes the call capturable without an allocation)."""
    _chk(disp)
    if not (disp.dim() == 3 or (disp.dim() == 4 and disp.shape[1] == 1)):
        raise RuntimeError('disp_densify: disp (n, 1, H, W) or (n, H, W) is expected')
    n, h, w = int(disp.shape[0]), int(disp.shape[-2]), int(disp.shape[-1])
    max_gap, min_dirs, max_spread, median = int(max_gap), int(min_dirs), float(max_spread), int(median)
    need = lib.fn('dis_disp_densify_workspace')(n, h, w)
    if need < 0:
        raise lib.DisHipError(f'dis_disp_densify_workspace: unsupported extents n={n} h={h} w={w}')
    if not (0 <= max_gap <= 32 and 1 <= min_dirs <= 8 and 0 <= median <= 2 and 0 <= max_spread <= 3.4028234663852886e38):
        # refused before anything is allocated or launched
        raise lib.DisHipError(f'disp_densify: unsupported configuration max_gap={max_gap} min_dirs={min_dirs} max_spread={max_spread} '
                              f'median={median}')
    dev = disp.device
    workspace = _workspace('disp_densify', need, workspace, dev)
    out = torch.empty_like(disp)
    state = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_state else None
    lib.call('dis_disp_densify', disp, out, state, n, h, w, max_gap, min_dirs, max_spread, median, workspace)
    return (out, state) if want_state else out


def flow_level_sizes(h, w, min_size=8):
    """[(h_0, w_0), (h_1, w_1), ...] of dis_dense_flow's pyramid: a further level while min(h, w) >= 2 min_size at the coarsest; every
    level halves the one before, rounding up"""
    sizes = [(int(h), int(w))]
    while min(sizes[-1]) >= 2 * int(min_size) and len(sizes) < 12:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def dense_flow(frames, alpha=1.0, warps=3, iters=64, min_size=8, workspace=None, want_debug=False, debug_level=0, variant=0):
    """dis_dense_flow: the flow between every ordered pair of the frames (n, tl, H, W) or (n, tl, 1, H, W) of n tracks ->
    (n, tl * tl, 2, H, W) fp32, entry i * tl + j the flow from frame i to frame j (channel 0 along x), zeros on the diagonal: the
    `_flow_stacked` layout of the workers.  Coarse-to-fine Horn-Schunck with warping (include/dis_hip.h, section "dense optical flow";
    tests/flow_ref.py restates it in numpy): alpha > 0 weighs the smoothness term, `warps` (1 .. 16) linearisations per level of
    `iters` (1 .. 1024) Jacobi steps each, a pyramid level per halving while min(h, w) >= 2 min_size (min_size >= 4); tl 2 .. 4,
    H and W 8 .. 8192.  want_debug: also a dict with pyr (list over the levels, finest first, of (n, tl, h_k, w_k)), levels (list of
    (n, tl (tl - 1), 2, h_k, w_k): the flow when level k is left) and warp ((4, n, tl (tl - 1), h, w): the warped second frame, Ix, Iy, It
    of the last warp at level debug_level).  variant 1: one launch per Jacobi step instead of 8 steps on an LDS-resident tile - the same
    values, for scripts/flow_rate.py.  The inputs are data: no autograd.  workspace: an optional uint8 tensor of at least
    dis_flow_workspace(...) bytes to reuse between calls (and what makes the call capturable without an allocation)."""
    _chk(frames)
    n, tl, h, w = _track_dims('dense_flow', frames, 'frames', 'are')
    alpha, warps, iters, min_size = float(alpha), int(warps), int(iters), int(min_size)
    need = lib.fn('dis_flow_workspace')(n, tl, h, w, min_size)
    if need < 0:
        raise lib.DisHipError(f'dis_flow_workspace: unsupported extents n={n} tl={tl} h={h} w={w} min_size={min_size}')
    sizes = flow_level_sizes(h, w, min_size)
    if not (0 < alpha < float('inf') and 1 <= warps <= 16 and 1 <= iters <= 1024 and variant in (0, 1)
            and 0 <= int(debug_level) < len(sizes)):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'dense_flow: unsupported configuration alpha={alpha} warps={warps} iters={iters} variant={variant} '
                              f'debug_level={debug_level}')
    dev = frames.device
    workspace = _workspace('dense_flow', need, workspace, dev)
    flow =torch.empty((n, tl * tl, 2, h, w), dtype=torch.float32, device=dev)
    D = lib.FlowDebug()
    D.level, D.variant = int(debug_level), int(variant)
    bufs = None
    if want_debug:
        P = n * tl * (tl - 1)
        bufs = {'pyr': torch.empty(sum(n * tl * a * b for a, b in sizes), dtype=torch.float32, device=dev),
                'levels': torch.empty(sum(P * 2 * a * b for a, b in sizes), dtype=torch.float32, device=dev),
                'warp': torch.empty((4, n, tl * (tl - 1)) + sizes[int(debug_level)], dtype=torch.float32, device=dev)}
        for k_, t_ in bufs.items():
            setattr(D, k_, t_.data_ptr())
    lib.call('dis_dense_flow', frames, flow, _ct.addressof(D), n, tl, h, w, alpha, warps, iters, min_size, workspace)
    if not want_debug:
        return flow
    dbg = {'warp': bufs['warp'], 'pyr': [], 'levels': []}
    o1 = o2 = 0
    for a, b in sizes:
        dbg['pyr'].append(bufs['pyr'][o1:o1 + n * tl * a * b].view(n, tl, a, b))
        dbg['levels'].append(bufs['levels'][o2:o2 + P * 2 * a * b].view(n, tl * (tl - 1), 2, a, b))
        o1 += n * tl * a * b
        o2 += P * 2 * a * b
    return flow, dbg


# ----------------------------------------------------------------------------------------------------------------------
# track fusion (csrc/fuse.hip; data/fuse.py writes the point clouds)
# ----------------------------------------------------------------------------------------------------------------------
def fuse_track(disp, R, t, K, baseline, value=None, tol=0.01, min_views=2, cap=None, workspace=None, want_dense=False):
    """dis_fuse_track: the disparity maps disp (n, tl, H, W) or (n, tl, 1, H, W) of n tracks with the poses R (n, tl, 3, 3), t (n, tl, 3)
    (X_c = R X_w + t), intrinsics K (3 x 3, host: numpy or a CPU tensor) and the baseline -> one point cloud per track in world
    coordinates (include/dis_hip.h, section "track fusion"; tests/fuse_ref.py restates it in numpy).  A pixel is valid where its
    disparity is finite and > 0; it is consistent with another frame where its point, projected there, meets that frame's depth within
    the relative tolerance tol in (0, 1).  A pixel is kept when it is consistent with at least min_views - 1 other frames (1 <= min_views
    <= tl) and with no earlier one.  value: an optional (n, tl, H, W) or (n, tl, 1, H, W) plane carried along (the ambient image).
    -> a dict of device tensors: xyz (cap, 3), normal (cap, 3), value (cap) fp32, src (cap) int32 (the linear index of the pixel in
    disp), count (n) int32.  The records are in ascending src; track b's start at count[:b].sum(); rows at and beyond count.sum() are
    not written.  cap (default n tl H W: everything fits) bounds the records written, count reports the true numbers.  want_dense: also
    views, seen, keep (n, tl, H, W) uint8, resid (n, tl, H, W) and point, dnormal (n, tl, 3, H, W) fp32.  The inputs are data: no
    autograd.  Three launches on the current stream, no synchronisation; workspace: an optional uint8 tensor of at least
    dis_fuse_workspace(...) bytes to reuse between calls (and what makes the call capturable without an allocation besides the
    outputs)."""
    _chk(disp, R, t)
    if value is not None:
        _chk(value)
    n, tl, h, w = _track_dims('fuse_track', disp)
    if tuple(R.shape) != (n, tl, 3, 3) or tuple(t.shape) != (n, tl, 3):
        raise RuntimeError('fuse_track: R (n, tl, 3, 3) and t (n, tl, 3) are expected')
    if value is not None and (value.numel() != disp.numel() or tuple(value.shape[:2]) != (n, tl) or tuple(value.shape[-2:]) != (h, w)):
        raise RuntimeError('fuse_track: value must have the shape of disp')
    need = lib.fn('dis_fuse_workspace')(n, tl, h, w)
    if need < 0:
        raise lib.DisHipError(f'dis_fuse_workspace: unsupported extents n={n} tl={tl} h={h} w={w}')
    tol, min_views, baseline = float(tol), int(min_views), float(baseline)
    K4 = _k4(K)
    total = n * tl * h * w
    cap = total if cap is None else int(cap)
    if not (0.0 < tol < 1.0 and 1 <= min_views <= tl and cap >= 0 and all(_fin(v) for v in K4) and K4[0] > 0 and K4[1] > 0
            and _fin(baseline) and baseline > 0):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'fuse_track: unsupported configuration tol={tol} min_views={min_views} cap={cap} K={K4} baseline={baseline}')
    dev = disp.device
    workspace = _workspace('fuse_track', need, workspace, dev)
    res = {'xyz': torch.empty((cap, 3), dtype=torch.float32, device=dev), 'normal': torch.empty((cap, 3), dtype=torch.float32, device=dev),
           'value': torch.empty((cap,), dtype=torch.float32, device=dev), 'src': torch.empty((cap,), dtype=torch.int32, device=dev),
           'count': torch.empty((n,), dtype=torch.int32, device=dev)}
    dense = {k_: torch.empty((n, tl, h, w), dtype=torch.uint8, device=dev) for k_ in ('views', 'seen', 'keep')}
    dense['resid'] = torch.empty((n, tl, h, w), dtype=torch.float32, device=dev)
    if want_dense:
        dense['point'] = torch.empty((n, tl, 3, h, w), dtype=torch.float32, device=dev)
        dense['dnormal'] = torch.empty((n, tl, 3, h, w), dtype=torch.float32, device=dev)
    O = _out_struct(lib.FuseOut, {**res, **dense})
    lib.call('dis_fuse_track', disp, R, t, lib.host_floats(K4), baseline, value, tol, min_views, cap, _ct.addressof(O), n, tl, h, w,
             workspace, int(workspace.numel()))
    if want_dense:
        res.update(dense)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# track poses (csrc/pose.hip; data/presave_pose.py writes R and t into frames.npz)
# ----------------------------------------------------------------------------------------------------------------------
def track_poses(disp, flow, K, baseline, iters=6, scale=1.0, damping=0.0, min_corr=64, workspace=None):
    """dis_track_poses: the disparity maps disp (n, tl, H, W) or (n, tl, 1, H, W) of n tracks and the flows between their frames,
    flow (n, tl * tl, 2, H, W) in the layout of dense_flow (entry i * tl + j the flow from frame i to frame j, the diagonal is not read),
    with the intrinsics K (3 x 3, host: numpy or a CPU tensor) and the baseline -> the relative pose of every ordered pair of frames
    (include/dis_hip.h, section "track poses"; tests/pose_ref.py restates it in numpy): X_j = R_pair[b, i, j] X_i + t_pair[b, i, j].
    `iters` (1 .. 64) Gauss-Newton steps from the identity on the residual in (u, v, disparity) of frame j; after the first step the
    residuals are weighted by 1 / (1 + r^2 / scale^2)^2 (scale > 0, in pixels); damping >= 0 adds damping * diag(H) to the normal
    matrix; a pair with fewer than min_corr (>= 6) usable pixels, or a singular system, fails and keeps its last good state.
    -> a dict of device tensors: R_pair (n, tl, tl, 3, 3), t_pair (n, tl, tl, 3), stats (n, tl, tl, 4) fp32 = {pixels used, mean
    weight, weighted rms residual in pixels, status (1 ok, 0 failed)}; the diagonal holds the identity.  The inputs are data: no
    autograd.  2 (iters + 1) launches on the current stream, no synchronisation; workspace: an optional uint8 tensor of at least
    dis_pose_workspace(...) bytes to reuse between calls (and what makes the call capturable without an allocation besides the
    outputs)."""
    _chk(disp, flow)
    n, tl, h, w = _track_dims('track_poses', disp)
    if tuple(flow.shape) != (n, tl * tl, 2, h, w):
        raise RuntimeError('track_poses: flow (n, tl * tl, 2, H, W) is expected')
    need = lib.fn('dis_pose_workspace')(n, tl, h, w)
    if need < 0:
        raise lib.DisHipError(f'dis_pose_workspace: unsupported extents n={n} tl={tl} h={h} w={w}')
    iters, scale, damping, min_corr, baseline = int(iters), float(scale), float(damping), int(min_corr), float(baseline)
    K4 = _k4(K)
    if not (1 <= iters <= 64 and _fin(scale) and scale > 0 and _fin(damping) and damping >= 0 and min_corr >= 6 and all(_fin(v) for v in K4)
            and K4[0] > 0 and K4[1] > 0 and _fin(baseline) and baseline > 0):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'track_poses: unsupported configuration iters={iters} scale={scale} damping={damping} min_corr={min_corr} '
                              f'K={K4} baseline={baseline}')
    dev = disp.device
    workspace = _workspace('track_poses', need, workspace, dev)
    res = {'R_pair': torch.empty((n, tl, tl, 3, 3), dtype=torch.float32, device=dev),
           't_pair': torch.empty((n, tl, tl, 3), dtype=torch.float32, device=dev),
           'stats': torch.empty((n, tl, tl, 4), dtype=torch.float32, device=dev)}
    lib.call('dis_track_poses', disp, flow, lib.host_floats(K4), baseline, iters, scale, damping, min_corr, res['R_pair'], res['t_pair'],
             res['stats'], n, tl, h, w, workspace, int(workspace.numel()))
    return res


def refine_track_poses(disp, flow, K, baseline, R_init, t_init, pair_use=None, iters=6, scale=1.0, damping=0.0, min_corr=64,
                       workspace=None):
    """dis_refine_track_poses: disp, flow, K and baseline as in track_poses, with one world pose per frame to start from, R_init
    (n, tl, 3, 3), t_init (n, tl, 3) (X_c = R X_w + t) -> the poses refined jointly on the residuals of every used ordered pair, frame 0
    kept where it is (include/dis_hip.h, section "track poses"; tests/pose_joint_ref.py restates it in numpy).  pair_use: an optional
    (n, tl, tl) uint8 (or bool) device tensor, non-zero where the pair (i, j) is used - the status of track_poses, say; None: every
    pair.  `iters` (1 .. 64) Gauss-Newton steps on the 6 (tl - 1) system, every pass weighted by 1 / (1 + r^2 / scale^2)^2; damping >= 0
    adds damping * diag(A); a pair with fewer than min_corr (>= 6) usable pixels does not contribute to a pass; a track whose system is
    singular - a frame that no contributing pair touches - fails and keeps its last good state.
    -> a dict of device tensors: R (n, tl, 3, 3), t (n, tl, 3), pair_stats (n, tl, tl, 4) fp32 = {pixels used, mean weight, weighted rms
    residual in pixels, contributed} of the closing pass, track_stats (n, 4) = {contributing pairs, their pixels, their weighted rms
    residual, status (1 ok, 0 failed)}.  The inputs are data: no autograd.  2 (iters + 1) launches on the current stream, no
    synchronisation; workspace: an optional uint8 tensor of at least dis_pose_joint_workspace(...) bytes to reuse between calls (and
    what makes the call capturable without an allocation besides the outputs)."""
    _chk(disp, flow, R_init, t_init)
    n, tl, h, w = _track_dims('refine_track_poses', disp)
    if tuple(flow.shape) != (n, tl * tl, 2, h, w):
        raise RuntimeError('refine_track_poses: flow (n, tl * tl, 2, H, W) is expected')
    if tuple(R_init.shape) != (n, tl, 3, 3) or tuple(t_init.shape) != (n, tl, 3):
        raise RuntimeError('refine_track_poses: R_init (n, tl, 3, 3) and t_init (n, tl, 3) are expected')
    if pair_use is not None:
        if not (isinstance(pair_use, torch.Tensor) and pair_use.is_cuda and pair_use.dtype in (torch.uint8, torch.bool)
                and pair_use.is_contiguous() and tuple(pair_use.shape) == (n, tl, tl)):
            raise RuntimeError('refine_track_poses: pair_use must be a contiguous (n, tl, tl) uint8 or bool CUDA(HIP) tensor')
    need = lib.fn('dis_pose_joint_workspace')(n, tl, h, w)
    if need < 0:
        raise lib.DisHipError(f'dis_pose_joint_workspace: unsupported extents n={n} tl={tl} h={h} w={w}')
    iters, scale, damping, min_corr, baseline = int(iters), float(scale), float(damping), int(min_corr), float(baseline)
    K4 = _k4(K)
    if not (1 <= iters <= 64 and _fin(scale) and scale > 0 and _fin(damping) and damping >= 0 and min_corr >= 6 and all(_fin(v) for v in K4)
            and K4[0] > 0 and K4[1] > 0 and _fin(baseline) and baseline > 0):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'refine_track_poses: unsupported configuration iters={iters} scale={scale} damping={damping} '
                              f'min_corr={min_corr} K={K4} baseline={baseline}')
    dev = disp.device
    workspace = _workspace('refine_track_poses', need, workspace, dev)
    res = {'R': torch.empty((n, tl, 3, 3), dtype=torch.float32, device=dev), 't': torch.empty((n, tl, 3), dtype=torch.float32, device=dev),
           'pair_stats': torch.empty((n, tl, tl, 4), dtype=torch.float32, device=dev),
           'track_stats': torch.empty((n, 4), dtype=torch.float32, device=dev)}
    lib.call('dis_refine_track_poses', disp, flow, lib.host_floats(K4), baseline, R_init, t_init, pair_use, iters, scale, damping, min_corr,
             res['R'], res['t'], res['pair_stats'], res['track_stats'], n, tl, h, w, workspace, int(workspace.numel()))
    return res


# ----------------------------------------------------------------------------------------------------------------------
# disparity alignment (csrc/disp_align.hip; data/presave_pose.py --pairwise disp, data/presave_flow.py --source geometry)
# ----------------------------------------------------------------------------------------------------------------------
DISP_ALIGN_ITERS = (10, 6, 4, 4, 4, 4)   # steps per level, finest first


def disp_align_levels(h, w):
    """the default number of pyramid levels of disp_align_poses: a further halving while the next level keeps min(h, w) >= 24"""
    levels = 1
    while levels < 6 and min(int(h) >> levels, int(w) >> levels) >= 24:
        levels += 1
    return levels


def disp_align_level_sizes(h, w, levels):
    """[(h_0, w_0), (h_1, w_1), ...] of dis_disp_align_poses' pyramid: every level halves the one before, rounding down"""
    return [(int(h) >> l, int(w) >> l) for l in range(int(levels))]


def disp_align_poses(disp, K, baseline, levels=None, iters=None, scale=0.3, damping=0.0, min_corr=64, jump=0.15, workspace=None,
                     want_debug=False, debug_level=0):
    """dis_disp_align_poses: the disparity maps disp (n, tl, H, W) or (n, tl, 1, H, W) of n tracks with the intrinsics K (3 x 3, host:
    numpy or a CPU tensor) and the baseline -> the relative pose of every ordered pair of frames, from the disparity maps alone - no flow
    is read (include/dis_hip.h, section "disparity alignment"; tests/disp_align_ref.py restates it in numpy):
    X_j = R_pair[b, i, j] X_i + t_pair[b, i, j].  Direct coarse-to-fine alignment of frame i's disparity map onto frame j's: Gauss-Newton
    from the identity on the residual in disparity, over a pyramid of `levels` (1 .. 6; default: halved while min(h, w) >= 24 is kept)
    with iters[l] (0 .. 64, not all 0; finest first; default (10, 6, 4, 4, 4, 4)) steps at level l, the coarsest level first; after the
    first step the residuals are weighted by 1 / (1 + e^2 / scale^2)^2 (scale > 0, in pixels of disparity); a pixel is not used next to
    a relative disparity step of `jump` (in (0, 1)) or more, or where its residual exceeds 2 jump of the predicted disparity; damping >= 0
    adds damping * diag(H); a pair with fewer than min_corr (>= 6) usable pixels, or a singular system - a fronto-parallel plane -,
    fails and keeps its last good state.  The scene is taken to be static.
    -> a dict of device tensors: R_pair (n, tl, tl, 3, 3), t_pair (n, tl, tl, 3), stats (n, tl, tl, 4) fp32 = {pixels used, mean weight,
    weighted rms residual in pixels of disparity, status (1 ok, 0 failed)} as track_poses gives them; the diagonal holds the identity.
    want_debug: also a dict with pyr (list over the levels from 1, of (n, tl, h_l, w_l)), maps ((n, tl, h_l, w_l, 4) = D, Dx, Dy, good of
    level debug_level) and sums ((passes, n, tl, tl, 30) fp64: the 30 sums of every pass).  The inputs are data: no autograd.
    2 levels - 1 + 2 (sum(iters) + 1) launches on the current stream, no synchronisation; workspace: an optional uint8 tensor of at least
    dis_disp_align_workspace(...) bytes to reuse between calls (and what makes the call capturable without an allocation besides the
    outputs)."""
    _chk(disp)
    n, tl, h, w = _track_dims('disp_align_poses', disp)
    levels = disp_align_levels(h, w) if levels is None else int(levels)
    need = lib.fn('dis_disp_align_workspace')(n, tl, h, w, levels)
    if need < 0:
        raise lib.DisHipError(f'dis_disp_align_workspace: unsupported extents n={n} tl={tl} h={h} w={w} levels={levels}')
    iters = [int(v) for v in (DISP_ALIGN_ITERS[:levels] if iters is None else iters)]
    scale, damping, min_corr, jump, baseline = float(scale), float(damping), int(min_corr), float(jump), float(baseline)
    K4 = _k4(K)
    if not (len(iters) == levels and all(0 <= v <= 64 for v in iters) and sum(iters) > 0 and _fin(scale) and scale > 0 and _fin(damping)
            and damping >= 0 and min_corr >= 6 and 0.0 < jump < 1.0 and all(_fin(v) for v in K4) and K4[0] > 0 and K4[1] > 0
            and _fin(baseline) and baseline > 0 and 0 <= int(debug_level) < levels):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'disp_align_poses: unsupported configuration levels={levels} iters={iters} scale={scale} damping={damping} '
                              f'min_corr={min_corr} jump={jump} K={K4} baseline={baseline} debug_level={debug_level}')
    dev = disp.device
    workspace = _workspace('disp_align_poses', need, workspace, dev)
    res = {'R_pair': torch.empty((n, tl, tl, 3, 3), dtype=torch.float32, device=dev),
           't_pair': torch.empty((n, tl, tl, 3), dtype=torch.float32, device=dev),
           'stats': torch.empty((n, tl, tl, 4), dtype=torch.float32, device=dev)}
    D, bufs = None, None
    sizes = disp_align_level_sizes(h, w, levels)
    if want_debug:
        D = lib.DispAlignDebug()
        D.level = int(debug_level)
        bufs = {'pyr': torch.empty(max(1, sum(n * tl * a * b for a, b in sizes[1:])), dtype=torch.float32, device=dev),
                'maps': torch.empty((n, tl) + sizes[int(debug_level)] + (4,), dtype=torch.float32, device=dev),
                'sums': torch.empty((sum(iters) + 1, n, tl, tl, 30), dtype=torch.float64, device=dev)}
        for k_, t_ in bufs.items():
            setattr(D, k_, t_.data_ptr())
    lib.call('dis_disp_align_poses', disp, lib.host_floats(K4), baseline, levels, lib.host_ints(iters), scale, damping, min_corr, jump,
             res['R_pair'], res['t_pair'], res['stats'], _ct.addressof(D) if D is not None else None, n, tl, h, w, workspace,
             int(workspace.numel()))
    if not want_debug:
        return res
    dbg = {'maps': bufs['maps'], 'sums': bufs['sums'], 'pyr': []}
    o = 0
    for a, b in sizes[1:]:
        dbg['pyr'].append(bufs['pyr'][o:o + n * tl * a * b].view(n, tl, a, b))
        o += n * tl * a * b
    return res, dbg


def rigid_flow(disp, R, t, K, baseline, tol=0.01, want_visible=False):
    """dis_rigid_flow: the flow that the disparity maps disp (n, tl, H, W) or (n, tl, 1, H, W) and the frame poses R (n, tl, 3, 3),
    t (n, tl, 3) (X_c = R X_w + t) of n static tracks imply, with the intrinsics K (3 x 3, host) and the baseline -> (n, tl * tl, 2, H, W)
    fp32 in the `_flow_stacked` layout of dense_flow (entry i * tl + j the flow from frame i to frame j, channel 0 along x), zeros on the
    diagonal (include/dis_hip.h, section "disparity alignment"; tests/disp_align_ref.py restates it in numpy).  A pixel without a valid
    disparity (finite and > 0), or whose point lies behind camera j, gets zeros.  want_visible: also (n, tl * tl, H, W) uint8, 1 where the
    pixel's point falls inside frame j and frame j's disparity at the nearest pixel agrees with the point's within the relative
    tolerance tol in (0, 1) (fuse_track's).  The inputs are data: no autograd.  One launch on the current stream, no synchronisation,
    no workspace: capturable once the outputs exist."""
    _chk(disp, R, t)
    n, tl, h, w = _track_dims('rigid_flow', disp)
    if tuple(R.shape) != (n, tl, 3, 3) or tuple(t.shape) != (n, tl, 3):
        raise RuntimeError('rigid_flow: R (n, tl, 3, 3) and t (n, tl, 3) are expected')
    if lib.fn('dis_pose_workspace')(n, tl, h, w) < 0:   # the extents of track_poses
        raise lib.DisHipError(f'rigid_flow: unsupported extents n={n} tl={tl} h={h} w={w}')
    tol, baseline = float(tol), float(baseline)
    K4 = _k4(K)
    if not (0.0 < tol < 1.0 and all(_fin(v) for v in K4) and K4[0] > 0 and K4[1] > 0 and _fin(baseline) and baseline > 0):
        raise lib.DisHipError(f'rigid_flow: unsupported configuration tol={tol} K={K4} baseline={baseline}')   # before any allocation
    dev = disp.device
    flow = torch.empty((n, tl * tl, 2, h, w), dtype=torch.float32, device=dev)
    visible = torch.empty((n, tl * tl, h, w), dtype=torch.uint8, device=dev) if want_visible else None
    lib.call('dis_rigid_flow', disp, R, t, lib.host_floats(K4), baseline, tol, flow, visible, n, tl, h, w)
    return (flow, visible) if want_visible else flow


# ----------------------------------------------------------------------------------------------------------------------
# volumetric fusion (csrc/tsdf.hip, csrc/raycast.hip, csrc/tsdf_align.hip; data/mesh.py writes the meshes, data/raycast.py the per-frame
# maps, data/presave_pose.py --model refines the poses against the volume)
# ----------------------------------------------------------------------------------------------------------------------
def tsdf_integrate(disp, R, t, K, baseline, value=None, *, origin, voxel, trunc, grid):
    """dis_tsdf_integrate: the disparity maps disp (tl, H, W) or (tl, 1, H, W) of ONE track, 1 <= tl <= 4, with the poses R (tl, 3, 3),
    t (tl, 3) (X_c = R X_w + t), intrinsics K (3 x 3, host) and the baseline -> a truncated signed distance volume on the lattice
    origin + (i, j, k) voxel, grid = (nx, ny, nz), each extent in 2 .. 1024 (include/dis_hip.h, section "volumetric fusion";
    tests/tsdf_ref.py restates it in numpy).  Every lattice point is projected into every frame and reads the nearest pixel; a frame
    whose depth there lies more than trunc in front of the point is skipped, the others add min(sdf / trunc, 1) with weight 1.
    value: an optional (tl, H, W) or (tl, 1, H, W) plane carried along (the ambient image), averaged over the frames that see the
    point within trunc of their surface.  -> tsdf (nz, ny, nx) fp32 (1 where unobserved), weight (nz, ny, nx) uint8, vvalue
    (nz, ny, nx) fp32.  The inputs are data: no autograd.  One launch on the current stream, no workspace, no synchronisation."""
    _chk(disp, R, t)
    if value is not None:
        _chk(value)
    if not (disp.dim() == 3 or (disp.dim() == 4 and disp.shape[1] == 1)):
        raise RuntimeError('tsdf_integrate: disp (tl, H, W) or (tl, 1, H, W) of one track is expected')
    tl, h, w = int(disp.shape[0]), int(disp.shape[-2]), int(disp.shape[-1])
    if tuple(R.shape) != (tl, 3, 3) or tuple(t.shape) != (tl, 3):
        raise RuntimeError('tsdf_integrate: R (tl, 3, 3) and t (tl, 3) are expected')
    if value is not None and (value.numel() != disp.numel() or int(value.shape[0]) != tl or tuple(value.shape[-2:]) != (h, w)):
        raise RuntimeError('tsdf_integrate: value must have the shape of disp')
    nx, ny, nz = (int(g) for g in grid)
    voxel, trunc, baseline = float(voxel), float(trunc), float(baseline)
    origin = [float(origin[0]), float(origin[1]), float(origin[2])]
    K4 = _k4(K)
    if not (1 <= tl <= 4 and 2 <= h <= 8192 and 2 <= w <= 8192 and all(2 <= g <= 1024 for g in (nx, ny, nz))):
        raise lib.DisHipError(f'tsdf_integrate: unsupported extents tl={tl} h={h} w={w} grid={(nx, ny, nz)}')
    if not (all(_fin(v) for v in K4 + origin + [voxel, trunc, baseline]) and voxel > 0 and trunc > 0 and K4[0] > 0 and K4[1] > 0
            and baseline > 0):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'tsdf_integrate: unsupported configuration voxel={voxel} trunc={trunc} origin={origin} K={K4} '
                              f'baseline={baseline}')
    dev = disp.device
    tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    weight = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
    vvalue = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    lib.call('dis_tsdf_integrate', disp, R, t, lib.host_floats(K4), baseline, value, lib.host_floats(origin), voxel, trunc, tsdf, weight,
             vvalue, tl, h, w, nx, ny, nz)
    return tsdf, weight, vvalue


def tsdf_mesh(tsdf, weight, vvalue, origin, voxel, min_weight=1, vcap=None, fcap=None, workspace=None, want_dense=False):
    """dis_tsdf_mesh: the volume tsdf (nz, ny, nx) fp32, weight (nz, ny, nx) uint8, vvalue (nz, ny, nx) fp32 of tsdf_integrate -> an
    indexed triangle mesh by naive surface nets (include/dis_hip.h, section "volumetric fusion"; tests/tsdf_ref.py restates it in
    numpy): one vertex per cell whose eight corners have weight >= min_weight (1 .. 4) and differ in the sign of tsdf, one quad - two
    triangles, their normals towards free space - per lattice edge that crosses the surface between four such cells.
    -> a dict of device tensors: xyz (vcap, 3), normal (vcap, 3), value (vcap) fp32, views (vcap) uint8 (the smallest corner weight),
    cell (vcap) int32 (ascending linear cell indices), faces (fcap, 3) int32, count (2) int32 = the true numbers of vertices and
    triangles; want_dense: also vid (nz - 1, ny - 1, nx - 1) int32, the vertex id of every cell or -1.  Rows at or beyond a cap are not
    written, nor is a triangle that names a vertex >= vcap.  With vcap and fcap given the call is five launches on the current stream
    with no synchronisation, and capturable when a workspace (uint8, at least dis_tsdf_mesh_workspace(nx, ny, nz) bytes, 16-byte
    aligned) is given too.  A cap left None is found by a counting call first - which reads `count` back, so it synchronises - and
    the outputs are then exactly as long as the mesh.  The inputs are data: no autograd."""
    _chk(tsdf, vvalue)
    if not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.is_contiguous()):
        raise RuntimeError('tsdf_mesh: weight must be a contiguous CUDA(HIP) tensor: the HIP path is the only path')
    if tsdf.dim() != 3 or tuple(weight.shape) != tuple(tsdf.shape) or tuple(vvalue.shape) != tuple(tsdf.shape):
        raise RuntimeError('tsdf_mesh: tsdf, weight and vvalue (nz, ny, nx) are expected')
    if tsdf.dtype != torch.float32 or vvalue.dtype != torch.float32 or weight.dtype != torch.uint8:
        raise RuntimeError('tsdf_mesh: tsdf and vvalue are float32, weight is uint8')
    nz, ny, nx = (int(v) for v in tsdf.shape)
    need = lib.fn('dis_tsdf_mesh_workspace')(nx, ny, nz)
    if need < 0:
        raise lib.DisHipError(f'dis_tsdf_mesh_workspace: unsupported extents nx={nx} ny={ny} nz={nz}')
    voxel, min_weight = float(voxel), int(min_weight)
    origin = [float(origin[0]), float(origin[1]), float(origin[2])]
    if not (all(_fin(v) for v in origin + [voxel]) and voxel > 0 and 1 <= min_weight <= 4
            and (vcap is None or int(vcap) >= 0) and (fcap is None or int(fcap) >= 0)):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'tsdf_mesh: unsupported configuration voxel={voxel} origin={origin} min_weight={min_weight} vcap={vcap} '
                              f'fcap={fcap}')
    dev = tsdf.device
    workspace = _workspace('tsdf_mesh', need, workspace, dev)
    origin_h = lib.host_floats(origin)

    def run(vc, fc, dense):
        res = {'xyz': torch.empty((vc, 3), dtype=torch.float32, device=dev), 'normal': torch.empty((vc, 3), dtype=torch.float32, device=dev),
               'value': torch.empty((vc,), dtype=torch.float32, device=dev), 'views': torch.empty((vc,), dtype=torch.uint8, device=dev),
               'cell': torch.empty((vc,), dtype=torch.int32, device=dev), 'faces': torch.empty((fc, 3), dtype=torch.int32, device=dev),
               'count': torch.empty((2,), dtype=torch.int32, device=dev)}
        if dense:
            res['vid'] = torch.empty((nz - 1, ny - 1, nx - 1), dtype=torch.int32, device=dev)
        O = _out_struct(lib.TsdfMeshOut, res)
        lib.call('dis_tsdf_mesh', tsdf, weight, vvalue, origin_h, voxel, min_weight, vc, fc, _ct.addressof(O), nx, ny, nz, workspace,
                 int(workspace.numel()))
        return res

    if vcap is None or fcap is None:
        nv, nf = (int(v) for v in run(0, 0, False)['count'].tolist())
        vcap = nv if vcap is None else int(vcap)
        fcap = nf if fcap is None else int(fcap)
    return run(int(vcap), int(fcap), want_dense)


def tsdf_raycast(tsdf, weight, vvalue, origin, voxel, R, t, K, baseline, size, step=None, min_weight=1, workspace=None, variant=0):
    """dis_tsdf_raycast: the volume tsdf (nz, ny, nx) fp32, weight (nz, ny, nx) uint8, vvalue (nz, ny, nx) fp32 of tsdf_integrate read
    back in the nv cameras R (nv, 3, 3), t (nv, 3) (X_c = R X_w + t, 1 <= nv <= 64; any poses, not only the track's) with the intrinsics
    K (3 x 3, host), the baseline and the image size = (h, w) (include/dis_hip.h, section "volumetric fusion"; tests/raycast_ref.py
    restates it in numpy).  Every pixel's ray is sampled at the camera depths n step, n = 1, 2, ... (step: a length, default voxel, in
    voxel / 8 .. 8 voxel); the first sample whose trilinear tsdf is negative, after a valid non-negative one, gives the crossing.
    -> a dict of device tensors: disp (nv, h, w), the disparity of the crossing; normal (nv, 3, h, w), world axes, towards free space;
    value (nv, h, w), the trilinear vvalue; all 0 where the ray meets no surface from observed free space.  A sample counts only where
    the eight lattice points of its cell have weight >= min_weight (1 .. 4).  variant 0 skips free and unobserved space through a
    byte per cell and a count per brick of 8 x 8 x 8 cells, variant 1 is the plain march; both give the same bits.  Up to three
    launches on the current stream, no synchronisation; capturable when a workspace (uint8, at least
    dis_tsdf_raycast_workspace(nx, ny, nz) bytes, 16-byte aligned) is given.  The inputs are data: no autograd."""
    _chk(tsdf, vvalue, R, t)
    if not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.is_contiguous()):
        raise RuntimeError('tsdf_raycast: weight must be a contiguous CUDA(HIP) tensor: the HIP path is the only path')
    if tsdf.dim() != 3 or tuple(weight.shape) != tuple(tsdf.shape) or tuple(vvalue.shape) != tuple(tsdf.shape):
        raise RuntimeError('tsdf_raycast: tsdf, weight and vvalue (nz, ny, nx) are expected')
    if tsdf.dtype != torch.float32 or vvalue.dtype != torch.float32 or weight.dtype != torch.uint8:
        raise RuntimeError('tsdf_raycast: tsdf and vvalue are float32, weight is uint8')
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or tuple(t.shape) != (int(R.shape[0]), 3):
        raise RuntimeError('tsdf_raycast: R (nv, 3, 3) and t (nv, 3) are expected')
    nz, ny, nx = (int(v) for v in tsdf.shape)
    nv, h, w = int(R.shape[0]), int(size[0]), int(size[1])
    need = lib.fn('dis_tsdf_raycast_workspace')(nx, ny, nz)
    if need < 0 or not (1 <= nv <= 64 and 2 <= h <= 8192 and 2 <= w <= 8192):
        raise lib.DisHipError(f'tsdf_raycast: unsupported extents nv={nv} h={h} w={w} nx={nx} ny={ny} nz={nz}')
    voxel, baseline, min_weight, variant = float(voxel), float(baseline), int(min_weight), int(variant)
    step = voxel if step is None else float(step)
    origin = [float(origin[0]), float(origin[1]), float(origin[2])]
    K4 = _k4(K)
    if not (all(_fin(v) for v in K4 + origin + [voxel, baseline, step]) and voxel > 0 and K4[0] > 0 and K4[1] > 0 and baseline > 0
            and 1 <= min_weight <= 4 and voxel / 8 <= step <= 8 * voxel and variant in (0, 1)):   # refused before anything is allocated
        raise lib.DisHipError(f'tsdf_raycast: unsupported configuration voxel={voxel} step={step} origin={origin} K={K4} '
                              f'baseline={baseline} min_weight={min_weight} variant={variant}')
    dev = tsdf.device
    workspace = _workspace('tsdf_raycast', need, workspace, dev)
    res = {'disp': torch.empty((nv, h, w), dtype=torch.float32, device=dev), 'normal': torch.empty((nv, 3, h, w), dtype=torch.float32, device=dev),
           'value': torch.empty((nv, h, w), dtype=torch.float32, device=dev)}
    lib.call('dis_tsdf_raycast', tsdf, weight, vvalue, lib.host_floats(origin), voxel, min_weight, R, t, lib.host_floats(K4), baseline, step,
             variant, res['disp'], res['normal'], res['value'], nv, h, w, nx, ny, nz, workspace, int(workspace.numel()))
    return res


def tsdf_align_poses(tsdf, weight, origin, voxel, trunc, disp, K, baseline, R_init, t_init, iters=6, scale=None, damping=0.0, min_corr=64,
                     min_weight=1, workspace=None):
    """dis_tsdf_align_poses: frame-to-model pose refinement.  The volume tsdf (nz, ny, nx) fp32, weight (nz, ny, nx) uint8 of
    tsdf_integrate on the lattice origin, voxel with the truncation distance trunc, and nv views - disp (nv, H, W) or (nv, 1, H, W)
    with the poses R_init (nv, 3, 3), t_init (nv, 3) (X_c = R X_w + t, 1 <= nv <= 64), intrinsics K (3 x 3, host) and the baseline -> the
    pose of every view refined on the signed distance of its back-projected pixels to the volume's surface (include/dis_hip.h,
    section "volumetric fusion"; tests/tsdf_align_ref.py restates it in numpy).  No flow is read.  A pixel is used where its disparity
    is valid, its point lies in a cell whose eight lattice points have weight >= min_weight (1 .. 4) and the trilinear tsdf there is
    inside (-1, 1).  `iters` (1 .. 64) Gauss-Newton steps, every pass weighted by 1 / (1 + e^2 / scale^2)^2 (scale: a length, default
    trunc / 2); damping >= 0 adds damping * diag(H); a view with fewer than min_corr (>= 6) used pixels, or a singular system, fails and
    keeps its last good state - R_init, t_init bit for bit if it fails in the first pass.  The start must lie within about the
    truncation band of the answer.
    -> a dict of device tensors: R (nv, 3, 3), t (nv, 3), stats (nv, 8) fp32 = {pixels used, mean weight, weighted rms residual (a
    length), status (1 ok, 0 failed)} of the closing pass, {pixels used, mean weight, weighted rms residual} of the opening pass at
    R_init, and the number of valid disparities.  A view's result does not depend on the other views of the call.  The inputs are
    data: no autograd.  2 (iters + 1) launches on the current stream, no synchronisation; workspace: an optional uint8 tensor of at
    least dis_tsdf_align_workspace(nv, H, W) bytes to reuse between calls (and what makes the call capturable without an allocation
    besides the outputs)."""
    _chk(tsdf, disp, R_init, t_init)
    if not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.is_contiguous()):
        raise RuntimeError('tsdf_align_poses: weight must be a contiguous CUDA(HIP) tensor: the HIP path is the only path')
    if tsdf.dim() != 3 or tuple(weight.shape) != tuple(tsdf.shape):
        raise RuntimeError('tsdf_align_poses: tsdf and weight (nz, ny, nx) are expected')
    if weight.dtype != torch.uint8:
        raise RuntimeError('tsdf_align_poses: tsdf is float32, weight is uint8')
    if not (disp.dim() == 3 or (disp.dim() == 4 and disp.shape[1] == 1)):
        raise RuntimeError('tsdf_align_poses: disp (nv, H, W) or (nv, 1, H, W) is expected')
    nv, h, w = int(disp.shape[0]), int(disp.shape[-2]), int(disp.shape[-1])
    if tuple(R_init.shape) != (nv, 3, 3) or tuple(t_init.shape) != (nv, 3):
        raise RuntimeError('tsdf_align_poses: R_init (nv, 3, 3) and t_init (nv, 3) are expected')
    nz, ny, nx = (int(v) for v in tsdf.shape)
    need = lib.fn('dis_tsdf_align_workspace')(nv, h, w)
    if need < 0 or not all(2 <= g <= 1024 for g in (nx, ny, nz)):
        raise lib.DisHipError(f'tsdf_align_poses: unsupported extents nv={nv} h={h} w={w} nx={nx} ny={ny} nz={nz}')
    voxel, trunc, baseline, damping = float(voxel), float(trunc), float(baseline), float(damping)
    iters, min_corr, min_weight = int(iters), int(min_corr), int(min_weight)
    scale = trunc / 2 if scale is None else float(scale)
    origin = [float(origin[0]), float(origin[1]), float(origin[2])]
    K4 = _k4(K)
    if not (all(_fin(v) for v in K4 + origin + [voxel, trunc, baseline, scale, damping]) and voxel > 0 and trunc > 0 and scale > 0
            and damping >= 0 and K4[0] > 0 and K4[1] > 0 and baseline > 0 and 1 <= iters <= 64 and min_corr >= 6
            and 1 <= min_weight <= 4):   # refused before anything is allocated or launched
        raise lib.DisHipError(f'tsdf_align_poses: unsupported configuration voxel={voxel} trunc={trunc} origin={origin} K={K4} '
                              f'baseline={baseline} iters={iters} scale={scale} damping={damping} min_corr={min_corr} '
                              f'min_weight={min_weight}')
    dev = disp.device
    workspace = _workspace('tsdf_align_poses', need, workspace, dev)
    res = {'R': torch.empty((nv, 3, 3), dtype=torch.float32, device=dev), 't': torch.empty((nv, 3), dtype=torch.float32, device=dev),
           'stats': torch.empty((nv, 8), dtype=torch.float32, device=dev)}
    lib.call('dis_tsdf_align_poses', tsdf, weight, lib.host_floats(origin), voxel, trunc, min_weight, disp, lib.host_floats(K4), baseline,
             R_init, t_init, iters, scale, damping, min_corr, res['R'], res['t'], res['stats'], nv, h, w, nx, ny, nz, workspace,
             int(workspace.numel()))
    return res
