"""Autograd operators over the C-ABI of include/nlam_hip.h.

PyTorch is used for device memory (caching allocator), the current HIP stream
and the autograd graph; every FLOP of the hot path runs in libnlam_hip.so.
There is deliberately no eager / CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from dataclasses import dataclass, field

import torch

from . import _lib as L


def _vec_stride(hid: int, dout: int) -> int:
    """Row stride of the (db1, db2, dgamma, dbeta) partial-sum buffer: a multiple of 64 >= max(hid, dout)."""
    return max(64, (max(hid, dout) + 63) // 64 * 64)



# Matrix path of the fused kernels (include/nlam_hip.h NLAM_F_MM_*): "f32" = fp32 MFMA (exact fmaf
# chains), "bf16x3" / "bf16x2" = operands split into 3 / 2 bf16 terms on the bf16 matrix cores with fp32
# accumulation (fp32-class / ~2^-16 product error), "bf16" = plain bf16 operands.
_MM_FLAGS = {"f32": 0, "bf16": 1 << 8, "bf16x2": 2 << 8, "bf16x3": 3 << 8}
MATMUL_MODE = os.environ.get("NLAM_MATMUL", "bf16x3")


def set_matmul_mode(mode: str, bwd: str | None = None):
    """``bwd``: matrix mode of the narrow backward launches under a "bf16x3" forward ("bf16x2" / "bf16x3"); None keeps it."""
    global MATMUL_MODE, MATMUL_MODE_BWD
    if mode not in _MM_FLAGS or (bwd is not None and bwd not in ("bf16x2", "bf16x3")):
        raise ValueError(f"unknown matmul mode {mode!r} / {bwd!r}; one of {sorted(_MM_FLAGS)}")
    MATMUL_MODE = mode
    if bwd is not None:
        MATMUL_MODE_BWD = bwd


def matmul_mode_name() -> str:
    """The modes in force outside autocast, for reports (bench.py's ``matmul_mode``)."""
    if MATMUL_MODE == "bf16x3" and MATMUL_MODE_BWD == "bf16x2":
        return "bf16x3 (narrow backward launches, d <= 64: bf16x2)"
    return MATMUL_MODE


# Matrix mode of the BACKWARD launches of the NARROW kernels (d <= 64: mlp_bwd_fast_kernel, the grouped embedder backward) when
# the forward runs in the default "bf16x3".  "bf16x2" = two bf16 terms per operand there (3 MFMAs per product block instead of 6, a
# third less splitting work and LDS weight image): OPT-IN, not the default.  VERDICT round 4 accepted two-term products as
# fp32-class (~2^-16 per operand against the TF32 the reference itself enables, train_model.py:484-488) PROVIDED every full-size
# parity test stays green at the unchanged tolerances.  Measured at cfg2 bench size (profiles/round5/parity_by_matmul_mode.log;
# bars 1e-4 / 1e-4 / 1e-4 / 1e-3):
#   forward / backward   prediction   loss      gradients (max-norm)   gradients (element-relative, row by row)   step
#   bf16x3 / bf16x3      2.2e-7       0         9.1e-6                 1.0e-4   <- default                         1.731-1.755 ms
#   bf16x3 / bf16x2      2.2e-7       0         2.1e-5                 6.9e-4                                      1.670-1.686 ms
#   bf16x2 / bf16x3      4.8e-6       1.1e-7    3.3e-5                 5.6e-4                                      1.724 ms
#   bf16x2 / bf16x2      4.8e-6       1.1e-7    3.0e-5                 1.08e-3  (fails the 1e-3 bar)               1.607 ms
# bf16x3 / bf16x2 holds every ONE-STEP bar with >= 30 % to spare, but fails test_cfg2_hip_graph_trainer_step_matches_oracle_adamw
# (weights after three AdamW steps against oracle + torch.optim.AdamW: 4.6e-4 against the 2e-4 bar -- Adam's first updates are
# lr * g / |g|, so gradient noise of 2e-5 of the largest element flips the step of elements that small): the condition is not
# met, the default stays three terms both ways.  NLAM_MATMUL_BWD=bf16x2 / set_matmul_mode(.., bwd="bf16x2") switch it on (-3.5 %).
MATMUL_MODE_BWD = os.environ.get("NLAM_MATMUL_BWD", "bf16x3")


def _bwd_flags(mm_flags: int, narrow: bool) -> int:
    """Matrix-path bits of the backward launches of a forward that ran with ``mm_flags``."""
    if (narrow and mm_flags == _MM_FLAGS["bf16x3"] and MATMUL_MODE_BWD in ("bf16x2", "bf16x3")
            and not torch.is_autocast_enabled("cuda")):
        return _MM_FLAGS[MATMUL_MODE_BWD]
    return mm_flags


def _bwd_pack(pack, mm_flags, bflags, *key):
    """The packer entry whose BACKWARD image has the backward's term count (``key`` = PACKER.get's arguments before the
    flags): the forward's own entry unless the two modes differ."""
    if pack is None or bflags == mm_flags or PACKER is None:
        return pack
    return PACKER.get(*key, bflags)


def _mm_flags() -> int:
    """Matrix-path bits for a launch.  Under ``torch.autocast`` (Lightning ``--precision bf16-mixed``,
    SURVEY.md section 8b "precision contract") the fused MLPs do what autocast does to the reference's
    ``nn.Linear``s: plain bf16 operands, fp32 accumulation, LayerNorm / SiLU / aggregation in fp32
    (fp16 autocast keeps two bf16 terms: at least fp16's 11 significant bits)."""
    if torch.is_autocast_enabled("cuda"):
        return _MM_FLAGS["bf16" if torch.get_autocast_dtype("cuda") == torch.bfloat16 else "bf16x2"]
    return _MM_FLAGS[MATMUL_MODE]


# bf16 STORAGE of what a fused MLP saves for / hands to its own backward (z1, xhat, dz1, dz2) inside a torch.autocast(bfloat16)
# region -- what Lightning's --precision bf16-mixed makes of the reference's nn.Linear outputs and their gradients
# (train_model.py:163-168) -- wherever the library has the kernels for it (nlam_store_bf16_supported: the one-term wide kernels).
STORE_BF16 = os.environ.get("NLAM_STORE_BF16", "1") == "1"


# When a trainer owns every parameter's .grad as a zero-initialised view of one flat buffer
# (trainer.FlatParams), the backward of a fused MLP adds its weight / bias / LayerNorm gradients straight
# into those views inside the partial-sum reduction and returns None for them: ~6 AccumulateGrad add
# launches per MLP (~130 per step at cfg2) disappear.  Off by default and only ever switched on for the duration
# of a trainer's own backward (``direct_param_grads()``): autograd's AccumulateGrad hooks -- which
# torch DistributedDataParallel / FSDP rely on -- are bypassed for those parameters while it is on.
DIRECT_PARAM_GRADS = False
# Object with ``note_use(params)`` / ``note_done(params)`` (trainer.GradBuckets): told, in direct mode, which
# parameters a forward used and when a backward has finished accumulating into their .grad, so that gradient
# buckets can be all-reduced as they complete although no AccumulateGrad hook fires.
GRAD_LISTENER = None


# Gradient hand-over inside one GNN layer (round 5).  A factorised layer consumes its receiver table x twice: as the input of
# the node-level products (NodeLinear[Pair]Function) and as source 0 (+ residual) of the node MLP.  Their backward passes used to
# return one (N, d) gradient each and autograd added the two: one `at::native add` launch per layer and AR step on the chain
# (120 launches, 4.9 ms of the cfg5 step).  Now the layer gives both consumers a private alias of x (so that no other consumer's
# gradient can meet theirs in autograd's input buffer) and a token; the node MLP's backward -- which runs first -- POSTS its dense
# source-0 gradient under the token, and the node-level product's backward ACCUMULATES into that buffer (nlam_linear with
# accumulate) and returns nothing.  Same two-operand fp32 additions, one launch fewer.  NLAM_GRAD_MAILBOX=0 switches it off.
GRAD_MAILBOX_ON = os.environ.get("NLAM_GRAD_MAILBOX", "1") == "1"
MAIL_TOKEN = None          # set by gnn_layers.InteractionNet.forward around its calls (mail_scope)
MAIL_ALIASED = None        # the token of a layer whose receiver table IS a private alias (set by InteractionNet.forward, read by consumers)
_MAIL_CONSUMERS = set()    # tokens for which a consumer (a node-level product, a twin edge launch) was recorded in this forward
_MAILBOX = {}              # token -> posted gradient buffer (B, N, w), between the two backward calls of one layer
MAIL_STATS = {"posted": 0, "consumed": 0}   # tests read it


@contextlib.contextmanager
def mail_scope():
    """Forward of ONE layer: the fused functions called inside record the token; yields it (None when switched off)."""
    global MAIL_TOKEN
    if not GRAD_MAILBOX_ON or not torch.is_grad_enabled():
        yield None
        return
    global MAIL_ALIASED
    prev, MAIL_TOKEN = MAIL_TOKEN, object()
    try:
        yield MAIL_TOKEN
    finally:
        _MAIL_CONSUMERS.discard(MAIL_TOKEN)
        MAIL_TOKEN = prev
        MAIL_ALIASED = None
        if len(_MAILBOX) > 256:   # posts whose consumer never ran (a backward that stopped half way): drop them
            _MAILBOX.clear()


# Tensors every autoregressive step of a rollout consumes as source 0 of a fused edge launch (the static edge embeddings, registered
# by models.compute_static_embeddings): addresses, and -- during backward -- the gradient buffer the first back-propagated step
# reported for each (see _fused_mlp_backward).  NLAM_ROLLOUT_ACC=0 switches the hand-over off.
ROLLOUT_ACC_ON = os.environ.get("NLAM_ROLLOUT_ACC", "1") == "1"
ROLLOUT_SHARED = {}       # address -> weak reference to the registered tensor (a dead tensor's address may be anybody's by now)
_ROLLOUT_USES = {}        # address -> fused launches of this forward pass that take the tensor as source 0 and have not been back-propagated
_ROLLOUT_ACC = {}         # address -> the gradient buffer their backward passes are collecting (held back until the last one)
ROLLOUT_ACC_STATS = {"accumulated": 0}   # tests read it


def rollout_shared_reset(tensors=()):
    """New rollout: register the tensors every AR step will consume.  A gradient buffer still held back from the previous pass
    means a consumer's backward never ran and the others' contributions were not reported: fail loudly."""
    if _ROLLOUT_ACC:
        _ROLLOUT_ACC.clear()
        _ROLLOUT_USES.clear()
        raise RuntimeError("gradient hand-over across a rollout: a consumer of a shared embedding was never back-propagated, the gradient "
                           "held back for it was not reported (set NLAM_ROLLOUT_ACC=0)")
    ROLLOUT_SHARED.clear()
    _ROLLOUT_ACC.clear()
    _ROLLOUT_USES.clear()
    import weakref

    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            ROLLOUT_SHARED[t.data_ptr()] = weakref.ref(t)


def _rollout_shared(t) -> bool:
    """``t`` (or a view of it starting at the same address) is a registered tensor that is still alive."""
    ref = ROLLOUT_SHARED.get(t.data_ptr())
    if ref is None:
        return False
    reg = ref()
    if reg is None:
        del ROLLOUT_SHARED[t.data_ptr()]
        return False
    return reg.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()


_MAIL_POST = False         # True only around the ONE launch that is a layer's node MLP (gnn_layers._node_update, single-launch depth)


@contextlib.contextmanager
def mail_post():
    global _MAIL_POST
    prev, _MAIL_POST = _MAIL_POST, True
    try:
        yield
    finally:
        _MAIL_POST = prev


# Early backward of "leaf" MLPs (see early_backward_leaf); switched on together with DIRECT_PARAM_GRADS.
EARLY_LEAF_BACKWARD = False


@contextlib.contextmanager
def direct_param_grads(listener=None, early_leaf=True, packer=None):
    global DIRECT_PARAM_GRADS, GRAD_LISTENER, EARLY_LEAF_BACKWARD, PACKER
    prev = (DIRECT_PARAM_GRADS, GRAD_LISTENER, EARLY_LEAF_BACKWARD, PACKER)
    DIRECT_PARAM_GRADS, GRAD_LISTENER, EARLY_LEAF_BACKWARD, PACKER = True, listener, bool(early_leaf), packer
    try:
        if packer is not None:
            packer.begin_step()   # the weight images of every registered MLP, rewritten from the current weights
        yield
    finally:
        DIRECT_PARAM_GRADS, GRAD_LISTENER, EARLY_LEAF_BACKWARD, PACKER = prev


def early_backward_leaf(out, force: bool = False):
    """Cut the autograd graph behind an MLP whose inputs need no gradient (the embedders of the static grid / mesh /
    edge features, the grid embedder of the first AR step) and run its backward as soon as the gradient of its output
    is complete, instead of when the autograd engine gets to it.

    The engine executes backward nodes in reverse order of their creation, so these first-created MLPs come last: at
    cfg2 their five data-gradient launches (86 + 41 + 45 + 33 + 21 us) formed a serial 270 us tail of the step although
    e.g. the gradient of the m2g edge embedding is final 900 us earlier.  Nothing downstream depends on them -- only
    the optimizer needs their parameter gradients -- so the consumer sees a detached leaf, and the leaf's
    post-accumulate hook (AccumulateGrad nodes have top priority in the engine) runs the MLP's own backward right
    there; FusedMLPFunction.backward puts all of it (data-gradient kernel included) on a weight-gradient side stream.
    """
    # ``force``: the caller knows the early launch pays (round 6: the m2g edge embedder inside the grouped launch, whose backward
    # then leaves the tail of the step) -- still only inside a trainer's own step (DIRECT_PARAM_GRADS), where the embedder's
    # whole backward goes to a side stream
    if not ((EARLY_LEAF_BACKWARD or (force and DIRECT_PARAM_GRADS)) and torch.is_grad_enabled() and out.requires_grad):
        return out
    leaf = out.detach().requires_grad_()

    def hook(t):
        g, t.grad = t.grad, None
        torch.autograd.backward(out, g)   # nested (re-entrant) backward of the small graph behind `out`

    leaf.register_post_accumulate_grad_hook(hook)
    return leaf


# ---- streams by hardware queue (round 6, DESIGN.md finding 54) -------------------------------------------------------------------
# ROCm runs all HIP streams of a process on a few in-order hardware queues (GPU_MAX_HW_QUEUES, default 4; a stream is bound to one
# when it is first used, whichever has the fewest streams then).  Which streams end up TOGETHER therefore depends on everything the
# process did before -- and a chain stream that shares its queue with weight-gradient side streams waits behind their launches: the
# same cfg3 step took 41.9 ms in a fresh process and 47.7 ms after a cfg2 trainer had run in it (profiles/round6/queue_placement.log:
# chain + two side streams on one queue, one queue idle).  The binding cannot be queried, but it can be OBSERVED: a tiny launch on
# stream b behind a spinning kernel on stream a finishes late exactly when the two share a queue.  stream_layout() does that once per
# process over a handful of pool streams and hands out a chain stream with a queue to itself and side streams spread over the others.
_LAYOUTS = {}   # device index -> layout
QUEUE_PROBE = os.environ.get("NLAM_QUEUE_PROBE", "1") == "1"
# side streams per hardware queue the chain does not use, in the order of the groups found; "0" = do not place anything (round-5
# behaviour: the next pool streams, wherever they land)
QUEUE_SIDES = os.environ.get("NLAM_QUEUE_SIDES", "")


def _streams_share_queue(a, b, tick, spin_cycles=6_000_000, attempts=3):
    """True when a launch on ``b`` waits for an earlier, long launch on ``a``: the two are bound to one in-order hardware queue.
    "The tiny launch finished while the spin was still running" cannot be observed by accident; "it finished after the spin" can
    (a host thread descheduled for 2 ms between the two launches): only ``attempts`` such observations in a row count as sharing."""
    for _ in range(attempts):
        torch.cuda.synchronize()
        ea, eb = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(a):
            torch.cuda._sleep(spin_cycles)   # ~2.5 ms
            ea.record()
        with torch.cuda.stream(b):
            tick.add_(1)
            eb.record()
        eb.synchronize()
        shared = ea.query()   # the spin was over before the tiny launch finished
        ea.synchronize()
        if not shared:
            return False
    return True


def stream_layout(nsides=None):
    """-> {"chain": stream, "sides": [streams], "groups": [[streams of one hardware queue], ..]} -- per device, built once per process."""
    dev = torch.cuda.current_device()
    if dev in _LAYOUTS:
        return _LAYOUTS[dev]
    lay = _stream_layout_build(nsides)
    if lay.pop("cache", True):
        _LAYOUTS[dev] = lay
    return lay


def _stream_layout_build(nsides):
    nsides = max(1, _WgradOverlap.NSTREAMS if nsides is None else nsides)
    if not QUEUE_PROBE or torch.cuda.is_current_stream_capturing():
        # never probe inside a capture; do not cache what was handed out there either
        return {"chain": torch.cuda.Stream(), "sides": [torch.cuda.Stream() for _ in range(nsides)], "groups": [],
                "cache": not torch.cuda.is_current_stream_capturing()}
    dev = torch.cuda.current_device()
    main = torch.cuda.default_stream()   # where a step is launched from (the first call comes from inside a trainer's warm-up stream)
    cands = [torch.cuda.Stream() for _ in range(12)]
    groups = [[main]]   # group 0 = the queue of the device's default stream
    try:
        tick = torch.zeros(1, device=f"cuda:{dev}")
        for c in cands:
            for g in groups:
                if _streams_share_queue(g[0], c, tick):
                    g.append(c)
                    break
            else:
                groups.append([c])
        torch.cuda.synchronize()
    except (AttributeError, RuntimeError) as exc:   # no spin kernel in this torch build, ...: unplaced streams, said once
        import warnings

        warnings.warn(f"hardware-queue probe failed ({exc!r}); the trainer's streams are not placed")
        return {"chain": cands[0], "sides": cands[1 : 1 + nsides], "groups": []}
    others = [g for g in groups[1:] if g]
    if not others:   # one queue for everything (GPU_MAX_HW_QUEUES=1): nothing to choose
        return {"chain": cands[0], "sides": cands[1 : 1 + nsides], "groups": groups}
    chain = others[0][0]
    # side queues: the ones neither the chain nor the caller uses.  Measured (profiles/round6/queue_placement.log): two side streams
    # on each of the two remaining queues 42.5 ms (cfg3) / 108.7 (cfg5) whatever ran in the process before; one of the four on the
    # caller's queue as well 45.9 / 115.7; three streams on three queues 43.6 / 110.1; unplaced 43.0 / 107.9 in a fresh process and
    # 48.5 / 124.0 after a cfg2 trainer.  NLAM_QUEUE_SIDES="a,b,c": a, b streams on those queues, c on the caller's.
    mine = [c for c in groups[0] if c is not main]
    side_groups = [g for g in others[1:] if g]
    if not side_groups:   # two queues in all: the side work shares the caller's
        side_groups = [mine] if mine else [others[0][1:] or [cands[-1]]]
    per_queue = [int(x) for x in QUEUE_SIDES.split(",")] if QUEUE_SIDES and QUEUE_SIDES != "0" else None
    sides = []
    if per_queue is not None:
        for g, n in zip([*others[1:], mine], per_queue):
            sides += g[:n]
    else:
        # neighbours in the list (= the side streams of MLPs whose backward passes follow each other) on the SAME queue: 42.0 against
        # 42.9 ms at cfg3 for the interleaved order
        per = -(-nsides // len(side_groups))
        for g in side_groups:
            sides += g[: min(per, nsides - len(sides))]
    if not sides:
        sides = [cands[-1]]
    # "comm": where a world > 1 step enqueues its waits for finished buckets -- on the default stream's queue, which carries nothing
    # between the batch copy and the optimizer: a stream that waits for side-graph events on the chain's (in-order) queue stalls the chain
    return {"chain": chain, "sides": sides, "groups": groups, "comm": mine[0] if mine else None}


WGRAD_SOLO_MODE = os.environ.get("NLAM_WGRAD_SOLO", "auto")   # "auto" | "0" (always the co-running shape) | "1" (always the solo shape)


@contextlib.contextmanager
def wgrad_shape(mode: str):
    """Pin the weight-gradient launch shape ("0" co-running, "1" solo) for the launches recorded inside, unless NLAM_WGRAD_SOLO already
    pins it.  trainer.graphed_training_step records its backward with the SOLO shape: the eager module it stands in for launches
    that shape, and the row-slice count decides the summation order of a weight gradient -- the two stay bit-identical."""
    global WGRAD_SOLO_MODE
    prev = WGRAD_SOLO_MODE
    if prev == "auto":
        WGRAD_SOLO_MODE = mode
    try:
        yield
    finally:
        WGRAD_SOLO_MODE = prev


def _wgrad_solo() -> int:
    """NLAM_F_WGRAD_SOLO for a weight gradient launched while no side streams are in use: nothing runs beside it.  Not while
    bench.py's roofline pass brackets launches with events (PROFILE: it times the shapes of the trainer's step, one by one) and
    not under WGRAD_SOLO_MODE "0" (tools/kernel_bench.py, the PMC passes: the same)."""
    if WGRAD_SOLO_MODE != "auto":
        return L.F_WGRAD_SOLO if WGRAD_SOLO_MODE == "1" else 0
    return 0 if (OVERLAP.active or PROFILE.enabled) else L.F_WGRAD_SOLO


class _WgradOverlap:
    """Weight-gradient kernels on a second HIP stream.

    The weight / bias / LayerNorm gradients of a fused MLP are needed only by the optimizer, not by the rest of
    backward, and at cfg2 sizes they are ~40 latency-bound launches per step.  While a trainer has this switched on
    (and owns the parameter gradients, DIRECT_PARAM_GRADS), FusedMLPFunction.backward forks them onto a side stream
    right after the data-gradient kernel; ``end()`` joins before the optimizer.  Inside a HIP-graph capture the fork /
    join become parallel branches of the graph.  Tensors the side stream reads are kept alive until the join."""

    NSTREAMS = int(os.environ.get("NLAM_WGRAD_STREAMS", "4"))

    def __init__(self):
        self.streams = []
        self.assigned = {}
        self.active = False
        self.capturing = False
        self.keep = []

    def begin(self, deferred=None):
        """``deferred``: an object with ``fork(k, fn, dead_end)`` / ``finish()`` (trainer._SegmentedCapture).  With it the side
        work is not launched here at all: every fork is handed over as (side-stream index, closure) and the trainer records
        it into graphs of its own, replayed beside the chain's (DESIGN.md finding 39)."""
        if not self.streams:
            # (CU-masked side streams -- hipExtStreamCreateWithCUMask -- were measured in round 6 and lose: DESIGN.md finding 47)
            self.streams = list(stream_layout()["sides"]) if QUEUE_SIDES != "0" else [torch.cuda.Stream() for _ in range(max(1, self.NSTREAMS))]
        self.active = True
        self.assigned = {}
        self.keep = []
        self.deferred = deferred
        self.capturing = torch.cuda.is_current_stream_capturing()
        WGRAD_BATCH.reset()

    deferred = None

    def index_for(self, owner):
        k = self.assigned.get(id(owner))
        if k is None:
            k = self.assigned[id(owner)] = len(self.assigned) % len(self.streams)
        return k

    def stream_for(self, owner):
        """Side streams are dealt round-robin over the fused MLPs in the order backward first meets them: on a single
        side stream the ~45 weight-gradient / reduction launches of a cfg2 step formed a 1.25 ms serial chain -- longer
        than the data-gradient chain they were moved off (rocprofv3 kernel trace of the replayed graph).  The stream is
        a function of the MLP (``owner`` = its first weight), not of the call: in a rollout the same parameters are
        back-propagated once per AR step, and the read-modify-write accumulations into one ``.grad`` must stay ordered
        on one stream (two streams = lost updates)."""
        return self.streams[self.index_for(owner)]

    def hold(self, side, *tensors):
        """Tensors the side stream reads must outlive its kernels.  Eager: ``record_stream`` hands that to the
        caching allocator (a block returns to the pool once the side stream has passed the point of release, not at
        the end of the whole backward).  During HIP-graph capture the private pool defers every cross-stream release
        to the end of the capture anyway; a plain reference until the join does the same without allocator events."""
        for t in tensors:
            if t is None:
                continue
            if self.capturing:
                self.keep.append(t)
            else:
                t.record_stream(side)

    def run(self, owner, hold, fn, dead_end=False):
        """``fn()`` (launches that read the tensors ``hold``) on ``owner``'s side stream, ordered behind everything enqueued on
        the current stream so far.  (Issuing the fork only after the chain's NEXT kernel was enqueued -- so that a captured
        graph keeps the chain on one hardware queue: the executor leaves a node's first child on the node's queue -- was
        measured in round 4: the chain did stay on one queue and lost its 12 us hop gaps, but every fork landed on ONE other
        queue in reverse order: cfg2 1.77 -> 2.08 ms; forks batched two to six at a time 1.89 - 2.02 ms.)"""
        if self.deferred is not None:
            # the tensors the closure reads stay referenced until every side graph has been recorded: inside the chain's
            # private pool a released block would be handed to a later chain kernel while the side graph still reads it
            self.keep.extend(t for t in hold if t is not None)
            self.deferred.fork(self.index_for(owner), fn, dead_end)
            return
        side = self.stream_for(owner)
        side.wait_stream(torch.cuda.current_stream())
        self.hold(side, *hold)
        with torch.cuda.stream(side):
            fn()

    def end(self):
        # the small weight gradients still waiting for company (WGRAD_BATCH) leave now: behind this point every gradient is
        # enqueued -- or, for a backward that failed (no longer active), dropped with the rest of its side work
        if self.active:
            try:
                WGRAD_BATCH.flush()
            except BaseException:
                self.deferred, self.keep, self.active = None, [], False
                raise
        WGRAD_BATCH.reset()
        if self.deferred is not None:
            d, self.deferred = self.deferred, None
            try:
                d.finish()
            finally:
                self.keep = []
                self.active = False
            return
        if self.active:
            for st in self.streams:
                torch.cuda.current_stream().wait_stream(st)
        self.keep = []
        self.active = False


OVERLAP = _WgradOverlap()


class WeightPacker:
    """Pre-packed weight images of the narrow fused kernels (``nlam_mlp_pack``), owned by a trainer.

    The reference's ``nn.Linear`` weights change once per optimizer step (models/module.py:293-304), but every workgroup of
    every fused-MLP launch used to read them as fp32 and split them into bf16 terms itself (~95 us of a 1.9 ms cfg2 step, on
    the critical path of ~30 latency-bound launches).  While a trainer has a packer installed (``direct_param_grads``), each
    fused MLP registers the image it needs the first time it runs; from the next step on ``begin_step`` rewrites ALL images
    with one launch and the kernels fetch them by LDS-DMA.  Keys are parameter addresses: the trainer's flat parameter
    buffer never moves."""

    def __init__(self):
        self.enabled = os.environ.get("NLAM_PACK_WEIGHTS", "1") == "1"
        self.entries = {}
        self.table = None          # device copy of the nlam_pack_job_t array
        self.table_entries = []    # the entries it describes, in table order
        self.dirty = False
        self.step_id = 0
        # wide launches (a width above 64): their `wpack` scratch, normally packed by a launch in front of every forward /
        # backward launch, lives in a persistent buffer per (MLP, launch geometry, direction) that nlam_pack_records fills
        # once per step from a table of pack records (one launch per record kind)
        self.wide_enabled = os.environ.get("NLAM_PACK_WIDE", "1") == "1"
        self.wide = {}
        self.wide_tables = {}      # kind -> (device table, [entries])
        self.wide_dirty = False
        # Tables a captured HIP graph may have baked into its nlam_mlp_pack / nlam_pack_records launches stay alive for the
        # packer's lifetime: entries registered AFTER a capture (a partial last batch taking the eager step registers wide
        # entries of another row count) rebuild the tables, and a replay of the older graph still reads the older ones --
        # freed, they would be read from recycled memory (raw source / destination pointers).  A table is <= a few KB.
        self._retired = []

    class Entry:
        __slots__ = ("job", "fwd", "bwd", "packed_step")

    class WideEntry:
        __slots__ = ("buf", "recs", "kind", "packed_step")

    def get(self, W1, W2, widths, hid, dout, pre, ldw1, mm_flags):
        """The entry whose images are valid for THIS step, or None (not served / registered only now)."""
        if not self.enabled:
            return None
        key = (W1.data_ptr(), W2.data_ptr(), tuple(widths), hid, dout, bool(pre), int(ldw1), int(mm_flags))
        e = self.entries.get(key)
        if e is None:
            job = L.PackJob()
            job.W1, job.W2, job.hid, job.dout, job.nsrc, job.ldw1 = W1.data_ptr(), W2.data_ptr(), hid, dout, len(widths), int(ldw1)
            for k, w in enumerate(widths):
                job.width[k] = int(w)
            job.flags = int(mm_flags) | (L.F_PRE_ADD if pre else 0)
            lib = L.load()
            nf, nb = int(lib.nlam_mlp_pack_floats(C.byref(job), 0)), int(lib.nlam_mlp_pack_floats(C.byref(job), 1))
            e = WeightPacker.Entry()
            e.job, e.fwd, e.bwd, e.packed_step = job, None, None, -1
            if nf > 0 and nb > 0:
                e.fwd = torch.empty((nf,), device=W1.device, dtype=torch.float32)
                e.bwd = torch.empty((nb,), device=W1.device, dtype=torch.float32)
                job.fwd_image, job.bwd_image = e.fwd.data_ptr(), e.bwd.data_ptr()
                self.dirty = True
            self.entries[key] = e
        return e if (e.fwd is not None and e.packed_step == self.step_id) else None

    def get_wide(self, which, p, nwp, key):
        """Persistent, already packed ``wpack`` buffer of the wide launch described by ``p`` (an MlpFwd for which = "f", an
        MlpBwd for "b"; every field but wpack filled), or None: not registered before this step (it is now), not served."""
        if not (self.enabled and self.wide_enabled):
            return None
        e = self.wide.get(key)
        if e is None:
            lib = L.load()
            e = WeightPacker.WideEntry()
            e.buf, e.recs, e.kind, e.packed_step = None, b"", -1, -1
            dev = torch.device("cuda", torch.cuda.current_device())
            buf = torch.empty((int(nwp),), device=dev, dtype=torch.float32)
            old = (p.wpack, p.wpack_floats)
            p.wpack, p.wpack_floats = buf.data_ptr(), int(nwp)
            recs, kind = (L.PackRec * 4)(), C.c_int32(-1)
            fn = lib.nlam_mlp_fwd_pack_records if which == "f" else lib.nlam_mlp_bwd_pack_records
            n = int(fn(C.byref(p), recs, 4, C.byref(kind)))
            p.wpack, p.wpack_floats = old
            if n > 0:
                e.buf, e.kind = buf, int(kind.value)
                e.recs = b"".join(bytes(recs[k]) for k in range(n))
                self.wide_dirty = True
            self.wide[key] = e
        return e.buf if (e.buf is not None and e.packed_step == self.step_id) else None

    def begin_step(self):
        """Rewrite every registered image from the current weights: one launch, first thing in the step (inside a captured
        step it is the first kernel of the graph).  Entries registered since the last call join the table here -- except
        during a stream capture (a host-to-device copy of the table is not capturable): they wait for the next eager call."""
        self.step_id += 1
        if not self.enabled:
            return
        if self.dirty and not torch.cuda.is_current_stream_capturing():
            live = [e for e in self.entries.values() if e.fwd is not None]
            arr = (L.PackJob * len(live))(*[e.job for e in live])
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            if self.table is not None:
                self._retired.append(self.table)
            self.table = host.to(live[0].fwd.device)
            self.table_entries = live
            self.dirty = False
        if self.table is not None:
            L.check(L.load().nlam_mlp_pack(C.c_void_p(self.table.data_ptr()), len(self.table_entries), _stream()), "nlam_mlp_pack")
            for e in self.table_entries:
                e.packed_step = self.step_id
        if self.wide_dirty and not torch.cuda.is_current_stream_capturing():
            by_kind = {}
            for e in self.wide.values():
                if e.buf is not None:
                    by_kind.setdefault(e.kind, []).append(e)
            self._retired.extend(t for t, _ in self.wide_tables.values())
            self.wide_tables = {}
            for kind, ents in by_kind.items():
                host = torch.frombuffer(bytearray(b"".join(e.recs for e in ents)), dtype=torch.uint8)
                self.wide_tables[kind] = (host.to(ents[0].buf.device), ents)
            self.wide_dirty = False
        for kind, (table, ents) in self.wide_tables.items():
            L.check(L.load().nlam_pack_records(C.c_void_p(table.data_ptr()), table.numel() // 64, kind, _stream()), "nlam_pack_records")
            for e in ents:
                e.packed_step = self.step_id


# Installed by a trainer for the duration of its own forward + backward (direct_param_grads)
PACKER = None


def _stream():
    d = OVERLAP.deferred
    if d is not None and d.cut_pending:   # trainer._SegmentedStep: a chain segment ends in front of this launch
        d.do_cut()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _LaunchProfile:
    """Optional HIP-event bracketing of individual kernel launches (bench.py's
    roofline leg).  Events are recorded on torch's current stream, which is the
    stream every launch of this module uses."""

    def __init__(self):
        self.enabled = False
        self._pairs = []
        self.meta = {}

    def reset(self, enabled: bool):
        self.enabled = enabled
        self._pairs = []
        self.meta = {}

    def launch(self, key, fn, meta=None):
        """``meta`` (a thunk, evaluated once per key and only while profiling): algorithmic FLOPs / HBM bytes of the launch
        and the matrix instruction it issues, for bench.py's roofline block."""
        if not self.enabled:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        self._pairs.append((key, e0, e1))
        if meta is not None and key not in self.meta:
            self.meta[key] = meta()
        return rc

    def collect(self):
        torch.cuda.synchronize()
        out = {}
        for key, e0, e1 in self._pairs:
            out.setdefault(key, []).append(e0.elapsed_time(e1))
        return out


PROFILE = _LaunchProfile()


def _ptr(t):
    """Device address of a tensor; None and raw addresses pass through."""
    return t.data_ptr() if isinstance(t, torch.Tensor) else t


_MM_NAMES = {0: "f32", 1: "bf16", 2: "bf16x2", 3: "bf16x3"}


def _mm_executed(mm_flags, hid, dout, widths, ragged_out_ok=False):
    """Matrix instruction a fused-MLP launch issues (mirrors the dispatch of csrc/nlam_hip.hip: shapes the split-bf16
    kernels do not cover run the fp32 MFMA) -> (name, bf16 MFMAs executed per algorithmic product block; 0 = fp32 MFMA)."""
    ns = (mm_flags >> 8) & 3
    covered = hid % 32 == 0 and (dout % 32 == 0 or (ragged_out_ok and dout < 32 and len(widths) == 1)) and all(w % 4 == 0 for w in widths)
    if max([hid, dout, *widths]) <= 64:
        covered = covered and (len(widths) == 1 or all(w % 32 == 0 for w in widths))
    if ns == 0 or not covered:
        return "f32", 0
    if max(hid, dout) > 64 and ns == 2:
        ns = 3
    return _MM_NAMES[ns], ns * (ns + 1) // 2


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "neural_lam_amd operators run on MI355X only: got a CPU tensor "
                "(there is no CPU/eager fallback; use the oracle/ package for a CPU reference)"
            )
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"neural_lam_amd operators are fp32: got {t.dtype}")


def as_batched(x: torch.Tensor):
    """(..., N, w) -> (tensor whose storage the kernel reads, B, bstride, lead_shape).

    A batch that is a stride-0 expansion (``StepPredictor.expand_to_batch``,
    step_predictors/base.py:122-139) is *not* materialised: the kernel gets
    bstride = 0 and reads the single copy.
    """
    lead = x.shape[:-2]
    N, w = x.shape[-2], x.shape[-1]
    B = 1
    for s in lead:
        B *= s
    if len(lead) > 0 and B > 1 and all(st == 0 for st, sz in zip(x.stride()[:-2], lead) if sz > 1):
        base = x[(0,) * len(lead)]
        if not base.is_contiguous():
            base = base.contiguous()
        return base, B, 0, lead
    xc = x if x.is_contiguous() else x.contiguous()
    return xc, B, N * w, lead


@dataclass
class MlpGeometry:
    """Static description of one fused-MLP call site (built once per module)."""

    nsrc: int
    flags: int = 0
    src_idx: list = field(default_factory=lambda: [None, None, None])  # int32 device tensors or None
    rows: int | None = None          # tile-rows per batch item (None: rows of source 0)
    tiles: torch.Tensor | None = None  # (ntiles, 4) int32 on device
    out_idx: torch.Tensor | None = None
    out_rows: int | None = None
    want_out: bool = True
    aggregate: bool = False
    rowptr: torch.Tensor | None = None
    inv_deg: torch.Tensor | None = None
    seg_of_row: torch.Tensor | None = None
    nseg_total: int = 0
    has_split: bool = False
    dmode: list = field(default_factory=lambda: [1, 1, 1])
    # for dmode == 2: CSC structure to finish the scatter-by-sender as a segment sum
    colptr: torch.Tensor | None = None
    cperm: torch.Tensor | None = None
    num_send: int = 0
    # receivers cut over several tiles (graph.build_tile_schedule, virtual split): rows of the aggregation / receiver-gradient
    # buffers including the virtual segments, and the (ptr, src, dst) lists of nlam_split_combine.  rowptr / inv_deg above are
    # then the extended arrays; nseg_total stays the number of REAL receivers.
    nseg_ext: int = 0
    comb: tuple | None = None
    # weights that are rewritten DURING the step (a padded copy made in forward): the trainer's once-per-step weight images would
    # be a step stale -- such a launch packs its weights itself
    no_pack: bool = False


def split_combine(buf, geom):
    """Second pass of the deterministic split-receiver reduction: sum the pieces (virtual rows of ``buf`` (B, nseg_ext, w)) into
    their receivers' rows, in place, fixed order."""
    ptr, src, dst = geom.comb
    B, _, w = buf.shape
    L.check(L.load().nlam_split_combine(_ptr(buf), buf.shape[1] * w, _ptr(ptr), _ptr(src), _ptr(dst), int(dst.numel()), w, B, _stream()),
            "nlam_split_combine")


def _fill_src(dst, tensor, bstride, width, idx):
    dst.ptr = _ptr(tensor)
    dst.idx = _ptr(idx)
    dst.bstride = bstride
    dst.width = width


def segment_sum(inp, in_bstride, ptr, order, scale, nseg, width, batch, out=None, accumulate=False):
    """out[b, s] (+)= scale[s] * sum_{q in ptr[s]:ptr[s+1]} inp[b, order[q]]"""
    _require_gpu(inp)
    if out is None:
        assert not accumulate
        out = torch.empty((batch, nseg, width), device=inp.device, dtype=torch.float32)
    fn = L.load().nlam_segment_sum_acc if accumulate else L.load().nlam_segment_sum
    rc = fn(
        _ptr(inp), in_bstride, _ptr(ptr), _ptr(order), _ptr(scale), _ptr(out), nseg, width, batch, _stream()
    )
    L.check(rc, "nlam_segment_sum")
    return out


def uses_gemm_family(hid: int, dout: int, widths) -> bool:
    """True when an MLP launch is wider than the fused kernels instantiate (nlam_max_width(): 512) and runs on the tiled-GEMM
    family (nlam_mlp_fwd_gemm / nlam_mlp_bwd_gemm) instead; narrower launches never do."""
    return max(int(hid), int(dout), *[int(w) for w in widths]) > _max_fused_width()


_MAX_FUSED = None


def _max_fused_width() -> int:
    global _MAX_FUSED
    if _MAX_FUSED is None:
        _MAX_FUSED = int(L.load().nlam_max_width())
    return _MAX_FUSED


def _gemm_ws(n: int, what: str) -> int:
    """A workspace query's answer: the floats, or the NLAM_E* code the launch would return (raised here, before any launch)."""
    if n < 0:
        L.check(int(n), what)
    return int(n)


def _gemm_mm(mm_flags):
    """Matrix instruction of a tiled-GEMM launch (PROFILE metadata): one bf16 term in the bf16 mode, three terms otherwise."""
    return ("bf16", 1) if (mm_flags >> 8) & 3 == 1 else ("bf16x3", 6)


# ---- from row gradients in HBM to dW / db / dgamma / dbeta: the one path every MLP backward takes ------------------------------------
# nlam_wgrad[_group] writes row-slice partial sums (_wgrad_request), nlam_reduce_jobs sums them in a fixed order (_ReduceBatch)
# either into a fresh tensor handed back to autograd or -- under a trainer, _direct_grad -- onto the parameter's .grad view.


def _direct_grad(param, shape) -> bool:
    """The gradient of ``param`` (of ``shape``) is accumulated straight into ``param.grad`` by the reduction launch instead of
    being returned to autograd: only in a trainer's direct mode, for a leaf whose .grad is a contiguous fp32 tensor of that shape.
    Under a trainer every parameter is a leaf whose .grad is an fp32 view of the flat gradient buffer with a matching shape: there
    this is simply "direct mode and .grad is set".  Every site that decides where a gradient lands, or whether an MLP's weight
    gradients may leave for a side stream, asks here, so that the two decisions cannot disagree."""
    return (DIRECT_PARAM_GRADS and param is not None and param.is_leaf and param.grad is not None and param.grad.is_contiguous()
            and tuple(param.grad.shape) == tuple(shape) and param.grad.dtype == torch.float32)


def _all_direct(params, needs) -> bool:
    """Every needed, non-None parameter of one MLP is direct for its own shape: nothing is returned to autograd."""
    return all(q is None or not nd or _direct_grad(q, q.shape) for q, nd in zip(params, needs))


class _ReduceBatch:
    """Jobs of nlam_reduce_jobs launches on the current stream: each sums ``nparts`` partial results in a fixed order."""

    def __init__(self, dev):
        self.jobs, self.keep, self.dev = L.ReduceJobs(), [], dev

    def reserve(self, n):
        """Room for ``n`` more jobs in the pending launch (the jobs of one MLP stay in one launch)."""
        if self.jobs.njobs + n > L.NLAM_MAX_REDUCE_JOBS:
            self.flush()

    def add(self, partials_ptr, nparts, stride, shape, param, *, ncols=0, out=None, out_off=0):
        """One job for the gradient of ``param`` (of ``shape``) -> (destination, direct).  Direct (_direct_grad): accumulated
        onto ``param.grad``; else written to a fresh tensor, which the caller returns to autograd.  ``ncols`` > 0: the partials
        are a (shape[0], ncols) column block of the matrix, written at column ``out_off`` (into ``out`` when several blocks share
        one destination; a fresh one is zeroed: the blocks need not cover it)."""
        direct = _direct_grad(param, shape)
        if out is None:
            out = param.grad if direct else (torch.zeros if ncols else torch.empty)(tuple(shape), device=self.dev, dtype=torch.float32)
        self.keep.append(out)
        self.reserve(1)
        j = self.jobs.job[self.jobs.njobs]
        j.partials, j.out, j.stride, j.nparts, j.accumulate = partials_ptr, out.data_ptr() + 4 * out_off, stride, nparts, 1 if direct else 0
        j.n, j.ncols, j.ld = (shape[0] * ncols, ncols, shape[1]) if ncols else (math.prod(shape), 0, 0)
        self.jobs.njobs += 1
        return out, direct

    def flush(self):
        if self.jobs.njobs > 0:
            L.check(L.load().nlam_reduce_jobs(C.byref(self.jobs), _stream()), "nlam_reduce_jobs")
            self.jobs.njobs = 0


def _mlp_reduce_jobs(batch, part1, part2, vecp, nblk, vs, vec_rows, dims, params, needs, has_ln, ncols=0):
    """The reduction jobs of one MLP's (dW1, db1, dW2, db2, dgamma, dbeta) -> the six results for autograd (None: not needed, or
    direct).  ``part1`` / ``part2``: (nparts, m, n) partial sums of dW1 (``ncols`` > 0: of its leading column block) / dW2, None =
    no job; the vector gradients are rows 0 .. 3 of the ``nblk`` blocks of ``vecp`` (``vec_rows`` rows of ``vs`` floats each)."""
    hid, kin, dout = dims
    res = [None] * 6
    mat = lambda part: (_ptr(part), part.shape[0], part.shape[1] * part.shape[2])   # noqa: E731  (nparts, m, n) partial sums
    vec = lambda r: (vecp.data_ptr() + r * vs * 4, nblk, vec_rows * vs)             # noqa: E731  row r of every block of vecp
    # (a padded dz2 gives (dpad, hid) partials of dW2: the first dout rows are the gradient)
    jobs = ((part1 is not None and mat(part1), (hid, kin)), (needs[1] and vec(0), (hid,)), (part2 is not None and mat(part2), (dout, hid)),
            (needs[3] and vec(1), (dout,)), (has_ln and needs[4] and vec(2), (dout,)), (has_ln and needs[5] and vec(3), (dout,)))
    for slot, (job, shape) in enumerate(jobs):
        if job:
            out, direct = batch.add(*job, shape, params[slot], ncols=ncols if slot == 0 else 0)
            if not direct:
                res[slot] = out
    return res


def _wgrad_request(A, m, n, B, rows, src_list, flags, dev):
    """-> (nlam_wgrad_t, partials) of dW (m, n) = A^T [sources]: ``A`` the (B * rows, m) row gradients, ``src_list`` entries
    (tensor | address, bstride, width, index tensor | address | None); ``partials`` (nparts, m, n) is what the launch writes."""
    q, nparts = _wgrad_describe(A, m, n, B, rows, src_list, flags)
    partials = torch.empty((nparts, m, n), device=dev, dtype=torch.float32)
    q.partials, q.nparts = _ptr(partials), nparts
    return q, partials


def _wgrad_describe(A, m, n, B, rows, src_list, flags):
    """-> (nlam_wgrad_t without its partials, nparts): what _wgrad_request launches, for questions about the launch's shape."""
    q = L.Wgrad()
    q.A, q.m, q.batch, q.rows, q.nsrc, q.flags, q.n = _ptr(A), m, B, rows, len(src_list), flags, n
    for k, (t, bstride, w, idx) in enumerate(src_list):
        _fill_src(q.src[k], t, bstride, w, idx)
    return q, L.load().nlam_wgrad_nparts(C.byref(q))


# ---- small narrow weight gradients, collected and launched together ----
# The node MLPs on the mesh (6 561 rows at cfg2) fork three launches each -- dW1, dW2, the reduction -- of which nearly all is
# fixed cost: one or two 32-row chunks per workgroup.  _WgradBatch collects such MLPs as backward meets them and launches K of
# them as ONE dW1 grid, ONE dW2 grid (nlam_wgrad_dma_group: members of one kernel shape, each computed as by its own launch) and
# ONE reduction.  Per member nothing changes -- nparts, chunks per workgroup, order of sums, order of the accumulations into one
# .grad -- so the gradients are the same bits.

WGRAD_BATCH_K = int(os.environ.get("NLAM_WGRAD_BATCH", "5"))   # members per flush; 0 = off (every MLP launches its own three)
# "small" = at most this many 32-row chunks per workgroup of the launch: where the fixed cost dominates (for measuring: 0 defers nothing)
WGRAD_BATCH_CHUNKS = int(os.environ.get("NLAM_WGRAD_BATCH_CHUNKS", "2"))


def wgrad_is_small(rows: int, batch: int, nparts: int, chunks_per_wg: int | None = None) -> bool:
    """A weight gradient over (batch, rows) rows on ``nparts`` workgroups is small when no workgroup sums more than
    ``chunks_per_wg`` (default WGRAD_BATCH_CHUNKS = 2) chunks of 32 rows: 6 561 rows are 206 chunks on 128 workgroups (yes), 57 616
    rows 1 801 on 226 (no)."""
    per = WGRAD_BATCH_CHUNKS if chunks_per_wg is None else chunks_per_wg
    return batch * ((rows + 31) // 32) <= per * nparts


def wgrad_batch_policy(pending_owners, pending_jobs: int, owner, njobs: int, k: int, cap: int | None = None, max_jobs: int | None = None):
    """When the collector flushes around the arrival of one MLP -> (flush before adding it, flush after adding it).
    ``pending_owners``: the owners (ids of the first weight) waiting, ``pending_jobs`` their reduction jobs; the arrival brings
    ``njobs``.  Before: its owner is already waiting (a rollout, gradient accumulation: two jobs adding into one .grad in one
    reduction launch would race, and the order of the sums per parameter is the order of back-propagation), or the grouped entry
    point's member cap / the reduction launch's job cap would be exceeded.  After: ``k`` members wait."""
    cap = L.NLAM_MAX_GROUP if cap is None else cap
    max_jobs = L.NLAM_MAX_REDUCE_JOBS if max_jobs is None else max_jobs
    before = len(pending_owners) > 0 and (owner in pending_owners or len(pending_owners) + 1 > cap or pending_jobs + njobs > max_jobs)
    waiting = (0 if before else len(pending_owners)) + 1
    return before, waiting >= min(max(k, 1), cap)


@dataclass
class _WgradMember:
    """One deferred MLP: what its three launches are made from (every tensor stays referenced here until the flush)."""

    owner: object
    B: int
    rows: int
    dims: tuple          # (hid, kin, dout)
    req1: tuple          # _wgrad_request arguments (A, m, n, src_list, flags) of dW1
    req2: tuple          # ... of dW2
    vecp: torch.Tensor
    nblk: int
    vs: int
    params: tuple
    needs: list
    has_ln: bool
    ncols: int
    njobs: int

    def tensors(self):
        out = [self.vecp]
        for A, _m, _n, src_list, _f in (self.req1, self.req2):
            out.append(A)
            out.extend(t for (t, _b, _w, _i) in src_list if isinstance(t, torch.Tensor))
        return out


class _WgradBatch:
    """The collector.  ``add`` is called from a fused MLP's backward in place of its fork; a flush is ONE OVERLAP.run closure.
    Every flush runs on one side stream (the collector is the closures' owner), so the accumulations into a parameter that is
    deferred more than once per step -- a rollout -- stay in the order of back-propagation."""

    def __init__(self):
        self.members = []
        self.seen = set()   # owners deferred since OVERLAP.begin(): their later launches of this step stay on the collector's stream

    def reset(self):
        self.members, self.seen = [], set()

    def enabled(self) -> bool:
        return WGRAD_BATCH_K > 0 and WGRAD_BATCH_CHUNKS > 0

    def wants(self, B, rows, req1, req2) -> bool:
        """Both launches are shapes the grouped entry point has, and small."""
        lib = L.load()
        for A, m, n, src_list, flags in (req1, req2):
            q, nparts = _wgrad_describe(A, m, n, B, rows, src_list, flags)
            if not lib.nlam_wgrad_dma_group_supported(C.byref(q)) or not wgrad_is_small(rows, B, nparts):
                return False
        return True

    def add(self, mem: _WgradMember):
        before, after = wgrad_batch_policy({id(m.owner) for m in self.members}, sum(m.njobs for m in self.members), id(mem.owner), mem.njobs, WGRAD_BATCH_K)
        if before:
            self.flush()
        self.members.append(mem)
        self.seen.add(id(mem.owner))
        if after:
            self.flush()

    def flush(self):
        members, self.members = self.members, []
        if members:
            OVERLAP.run(self, tuple(t for m in members for t in m.tensors()), lambda: _wgrad_batch_launch(members))


WGRAD_BATCH = _WgradBatch()


def _wgrad_batch_launch(members):
    """The launches of one flush, on the current (side) stream: per kernel shape one grouped launch (a shape with one member: its
    own nlam_wgrad), then the members' reductions in arrival order in one nlam_reduce_jobs launch, then the completion reports."""
    lib = L.load()
    dev = members[0].vecp.device
    parts, classes = [], {}
    for mem in members:
        got = []
        for A, m, n, src_list, flags in (mem.req1, mem.req2):
            q, partials = _wgrad_request(A, m, n, mem.B, mem.rows, src_list, flags, dev)
            key = (m, n, flags, tuple(w for (_t, _b, w, _i) in src_list))
            classes.setdefault(key, []).append((q, A, src_list, partials))
            got.append(partials)
        parts.append(got)
    for (m, n, _flags, _widths), reqs in classes.items():
        for g0 in range(0, len(reqs), L.NLAM_MAX_GROUP):
            grp = reqs[g0 : g0 + L.NLAM_MAX_GROUP]
            rc = -2
            if len(grp) > 1:
                arr = (L.Wgrad * len(grp))(*[r[0] for r in grp])
                rows_all = sum(int(r[0].rows) * int(r[0].batch) for r in grp)

                def meta(grp=grp, rows_all=rows_all, m=m, n=n):
                    nbytes = sum(A.numel() * 4 + p_.numel() * 4 + sum(t.shape[-2] * w * 4 for (t, _b, w, _i) in sl if isinstance(t, torch.Tensor))
                                 for (_q, A, sl, p_) in grp)
                    return {"flops": 2.0 * rows_all * m * n, "bytes": float(nbytes), "bytes_min": float(nbytes - sum(r[3].numel() * 4 for r in grp) + len(grp) * m * n * 4),
                            "mm": "f32", "mfmas_per_block": 0, "what": "weight gradients dW = A^T [gathered B] of several small MLPs in one grid"}

                rc = PROFILE.launch(("wgrad_dma_group", rows_all, len(grp), m, n), lambda: lib.nlam_wgrad_dma_group(arr, len(grp), _stream()), meta)
            if rc == -2:   # one member, or operands the DMA kernel cannot fetch (alignment): each on its own
                for r in grp:
                    L.check(PROFILE.launch(("wgrad", int(r[0].rows) * int(r[0].batch), m, n), lambda r=r: lib.nlam_wgrad(C.byref(r[0]), _stream())), "nlam_wgrad")
            else:
                L.check(rc, "nlam_wgrad_dma_group")
    batch = _ReduceBatch(dev)
    done = []
    for mem, (part1, part2) in zip(members, parts):
        batch.reserve(mem.njobs)
        _mlp_reduce_jobs(batch, part1, part2, mem.vecp, mem.nblk, mem.vs, 4, mem.dims, mem.params, mem.needs, mem.has_ln, ncols=mem.ncols)
        done.append([q for q, nd in zip(mem.params, mem.needs) if nd and q is not None and _direct_grad(q, q.shape)])
    batch.flush()
    OVERLAP.hold(torch.cuda.current_stream(), *[p_ for got in parts for p_ in got])
    if GRAD_LISTENER is not None:   # inside the side-stream context, as for an MLP that launches its own
        for d in done:
            GRAD_LISTENER.note_done(d)


@dataclass
class _WgradItem:
    """What the weight gradients of one fused MLP are computed from, once its data-gradient launch has written dz1 / dz2 / vecp."""

    B: int
    rows: int
    hid: int
    dout: int
    kin: int
    mm_flags: int
    dz1: torch.Tensor
    dz2: torch.Tensor
    z1: torch.Tensor
    vecp: torch.Tensor
    nblk: int
    vs: int
    src_list: list
    params: tuple
    needs: list
    has_ln: bool


def _wide_wpack(p, nwp, side, key, dev, use_packer=True):
    """Give the wide launch ``p`` (MlpFwd for side "f", MlpBwd for "b") its ``nwp`` floats of weights in MFMA A-operand order:
    the image the trainer's packer filled once for this step (``key``: its cache key), else scratch that the launch fills itself --
    returned, for the caller to keep alive; None otherwise."""
    wbuf = PACKER.get_wide(side, p, nwp, key) if (PACKER is not None and use_packer) else None
    if wbuf is not None:
        p.wpack, p.wpack_floats, p.flags = wbuf.data_ptr(), nwp, int(p.flags) | L.F_WPACK_READY
        return None
    wpack = torch.empty((nwp,), device=dev, dtype=torch.float32)
    p.wpack, p.wpack_floats = _ptr(wpack), nwp
    return wpack


def _unbatch_grad(g, shape, B):
    """The (B, ...) gradient of a source of ``shape``: summed over the batch when the source had no batch dimension of its own."""
    if math.prod(shape[:-2]) != B:
        g = g.sum(0) if B > 1 else g[0]
    return g.reshape(shape)


class FusedMLPFunction(torch.autograd.Function):
    """[gather|concat] -> Linear -> SiLU -> Linear -> [LayerNorm] -> residuals / aggregation.

    forward(geom, W1, b1, W2, b2, ln_w, ln_b, *sources) -> (out | None, aggr | None)
    """

    @staticmethod
    def forward(ctx, geom: MlpGeometry, W1, b1, W2, b2, ln_w, ln_b, *srcs):
        lib = L.load()
        assert len(srcs) == geom.nsrc
        mm_flags = _mm_flags()   # read before anything can change the autocast state; backward re-uses it
        if geom.flags & L.F_NO_ACT:
            mm_flags = 0   # Linear [-> LayerNorm] launches (hidden_layers = 0): the fp32 MFMA kernels carry the activation switch
        # storage is fp32 throughout: low-precision activations handed in by an autocast region are widened here
        srcs = tuple(s if s.dtype == torch.float32 or not s.is_floating_point() else s.float() for s in srcs)
        _require_gpu(W1, b1, W2, b2, ln_w, ln_b, *srcs)
        hid, kin = W1.shape
        dout = W2.shape[0]
        binfo = [as_batched(s) for s in srcs]
        B = max(bi[1] for bi in binfo)
        lead = max((bi[3] for bi in binfo), key=len)
        for (t, b_, _, _), s in zip(binfo, srcs):
            if b_ not in (1, B):
                raise RuntimeError(f"inconsistent batch sizes among sources: {b_} vs {B}")
        widths = [s.shape[-1] for s in srcs]
        pre = bool(geom.flags & L.F_PRE_ADD)   # factorised edge MLP: sources 1.. are pre-activation addends (width hid)
        if pre:
            if widths[0] > kin or any(w != hid for w in widths[1:]):
                raise RuntimeError(f"factorised edge MLP: source widths {widths} do not fit W1 {tuple(W1.shape)}")
        elif sum(widths) != kin:
            raise RuntimeError(f"source widths {widths} do not add up to the first Linear's in_features {kin}")
        rows = geom.rows if geom.rows is not None else srcs[0].shape[-2]
        ntiles = geom.tiles.shape[0] if geom.tiles is not None else (rows + 31) // 32
        dev = srcs[0].device
        need_grad = any(ctx.needs_input_grad[1:])
        gemm = uses_gemm_family(hid, dout, widths)   # wider than the fused kernels: the tiled-GEMM family (nlam_mlp_*_gemm)
        if gemm and pre:
            raise RuntimeError(f"factorised edge MLP at width {max(hid, dout, *widths)}: above nlam_max_width() the layer runs unfactorised")

        p = L.MlpFwd()
        for k in range(geom.nsrc):
            t, b_, bstride, _ = binfo[k]
            _fill_src(p.src[k], t, bstride if b_ == B or B == 1 else 0, widths[k], geom.src_idx[k])
        p.nsrc, p.batch, p.rows, p.ntiles = geom.nsrc, B, rows, ntiles
        p.tiles = _ptr(geom.tiles)
        W1c, b1c, W2c, b2c = W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()
        p.W1, p.b1, p.W2, p.b2 = _ptr(W1c), _ptr(b1c), _ptr(W2c), _ptr(b2c)
        p.ln_w, p.ln_b = _ptr(ln_w), _ptr(ln_b)
        p.eps, p.hid, p.dout, p.flags = 1e-5, hid, dout, geom.flags | mm_flags
        p.ldw1 = kin if pre else 0
        out = aggr = None
        if geom.want_out:
            out_rows = geom.out_rows if geom.out_rows is not None else rows
            out = torch.empty((B, out_rows, dout), device=dev, dtype=torch.float32)
            p.out, p.out_idx, p.out_bstride = _ptr(out), _ptr(geom.out_idx), out_rows * dout
        nseg_rows = geom.nseg_ext if geom.comb is not None else geom.nseg_total   # incl. the virtual segments of split receivers
        if geom.aggregate:
            alloc = torch.zeros if geom.has_split else torch.empty
            aggr = alloc((B, nseg_rows, dout), device=dev, dtype=torch.float32)
            p.aggr, p.rowptr, p.inv_deg, p.nseg_total = _ptr(aggr), _ptr(geom.rowptr), _ptr(geom.inv_deg), nseg_rows
        z1 = xhat = rstd = None
        sbf = False
        if need_grad:
            # saved tensors as bf16 rows: bf16 autocast only, where forward, backward and both weight gradients have the kernels
            sbf = (STORE_BF16 and not gemm and mm_flags == _MM_FLAGS["bf16"] and torch.is_autocast_enabled("cuda")
                   and bool(lib.nlam_store_bf16_supported(C.byref(p))))
            sdt = torch.bfloat16 if sbf else torch.float32
            if sbf:
                p.flags = int(p.flags) | L.F_STORE_BF16
            z1 = torch.empty((B, rows, hid), device=dev, dtype=sdt)
            p.z1 = _ptr(z1)
            if ln_w is not None:
                xhat = torch.empty((B, rows, dout), device=dev, dtype=sdt)
                rstd = torch.empty((B, rows), device=dev, dtype=torch.float32)
                p.xhat, p.rstd = _ptr(xhat), _ptr(rstd)
        ctx.store_bf16 = sbf
        ctx.gemm = gemm
        nwp = 0 if gemm else lib.nlam_mlp_fwd_wpack_floats(C.byref(p))
        bflags = mm_flags if gemm else _bwd_flags(mm_flags, narrow=nwp == 0)
        ctx.mm_flags = bflags   # backward reads nothing else
        pack = None
        if gemm:   # intermediates (z2 / messages) in a scratch of its own; the weights are read as they are, nothing is packed
            nws = _gemm_ws(lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p)), "nlam_mlp_fwd_gemm_workspace_floats")
            wpack = torch.empty((max(nws, 1),), device=dev, dtype=torch.float32)
            p.wpack, p.wpack_floats = _ptr(wpack), nws
        elif nwp > 0:  # wide kernels: the weights in MFMA A-operand order -- packed once per step under a trainer, else scratch the launch fills
            wpack = _wide_wpack(p, nwp, "f", ("f", W1c.data_ptr(), W2c.data_ptr(), tuple(widths), hid, dout, int(p.flags) & ~L.F_STORE_BF16, int(p.ldw1),
                                              rows, ntiles, B), dev, not geom.no_pack)
        elif PACKER is not None and mm_flags != 0 and not geom.no_pack:   # narrow split-bf16 kernels under a trainer: the image packed once for this step
            pack = PACKER.get(W1c, W2c, widths, hid, dout, pre, kin if pre else 0, mm_flags)
            if pack is not None:
                p.wpack, p.wpack_floats = pack.fwd.data_ptr(), pack.fwd.numel()
            pack = _bwd_pack(pack, mm_flags, bflags, W1c, W2c, widths, hid, dout, pre, kin if pre else 0)
        ctx.pack = pack
        key = ("mlp_fwd", rows * B, kin, hid, dout, geom.nsrc, bool(geom.aggregate), need_grad)

        def fwd_meta():
            # algorithmic HBM bytes: every distinct source row once (a gathered node table counts as the table), the
            # outputs, and in training mode the tensors saved for backward; weights / indices / descriptors are noise
            nbytes = sum(s_.shape[-2] * w_ * 4 * (B if bi[2] != 0 or B == 1 else 1) for s_, w_, bi in zip(srcs, widths, binfo))
            if out is not None:
                nbytes += out.numel() * 4
            if aggr is not None:
                nbytes += aggr.numel() * 4
            nmin = nbytes   # inputs once, outputs once -- nothing saved for a backward that could recompute it
            for t_ in (z1, xhat, rstd):
                if t_ is not None:
                    nbytes += t_.numel() * t_.element_size()
            name, mf = _gemm_mm(mm_flags) if gemm else _mm_executed(mm_flags, hid, dout, widths, ragged_out_ok=ln_w is None and not geom.aggregate)
            k1 = widths[0] if pre else kin
            return {"flops": 2.0 * rows * B * (k1 * hid + hid * dout), "bytes": float(nbytes), "bytes_min": float(nmin), "mm": name, "mfmas_per_block": mf,
                    "what": ("gather + " if geom.nsrc == 3 else "") + ("factorised " if pre else "") + "Linear-SiLU-Linear" + ("-LayerNorm" if ln_w is not None else "")
                            + (" + segment aggregate" if geom.aggregate else "") + (" (saves z1/xhat/rstd)" if need_grad else "")}

        fwd_fn = lib.nlam_mlp_fwd_gemm if gemm else lib.nlam_mlp_fwd
        L.check(PROFILE.launch(key, lambda: fwd_fn(C.byref(p), _stream()), fwd_meta), fwd_fn.__name__)
        if aggr is not None and geom.comb is not None:
            split_combine(aggr, geom)
            aggr = aggr[:, : geom.nseg_total]
            if B > 1:   # the real rows of a batch item are followed by its virtual rows: ONE compaction here instead of a copy in
                aggr = aggr.contiguous()   # every consumer (as_batched, the backward's reshape, the twin accumulation)

        if need_grad:
            ctx.geom, ctx.B, ctx.rows, ctx.ntiles = geom, B, rows, ntiles
            ctx.binfo = [(b_, bstride) for (_, b_, bstride, _) in binfo]
            ctx.src_shapes = [tuple(s.shape) for s in srcs]
            # a sender source (dmode 2) that is the very tensor also passed as the receiver source (dmode 3)
            ctx.twin_of = {}
            for k in range(geom.nsrc):
                for t in range(geom.nsrc):
                    if (t != k and geom.dmode[k] == 2 and geom.dmode[t] == 3 and srcs[k].data_ptr() == srcs[t].data_ptr()
                            and srcs[k].shape == srcs[t].shape and srcs[k].stride() == srcs[t].stride()
                            and ctx.needs_input_grad[7 + k] and ctx.needs_input_grad[7 + t]):
                        ctx.twin_of[k] = t
            # mesh <-> mesh layer run unfactorised (narrow widths): this launch's gradient of the node table (receiver side + sender
            # side) is accumulated onto the one the layer's node MLP posts (one nlam_segment_sum_add pass), nothing reported
            ctx.mail = None
            if ctx.twin_of and MAIL_TOKEN is not None and MAIL_ALIASED is MAIL_TOKEN:
                tw = next(iter(ctx.twin_of.values()))
                if len(ctx.twin_of) == 1 and (binfo[tw][1] == B or B == 1):
                    ctx.mail = MAIL_TOKEN
                    _MAIL_CONSUMERS.add(MAIL_TOKEN)
            ctx.has_ln = ln_w is not None
            # a tensor registered as shared by the AR steps of a rollout, taken as source 0 with a row-wise gradient: this launch is one of
            # the consumers whose backward passes collect its gradient in one buffer (see _fused_mlp_backward)
            ctx.acc_key = None
            if (ROLLOUT_ACC_ON and geom.dmode[0] == 1 and ctx.needs_input_grad[7] and ROLLOUT_SHARED and _rollout_shared(srcs[0])
                    and (binfo[0][1] == B or B == 1)):
                ctx.acc_key = srcs[0].data_ptr()
                _ROLLOUT_USES[ctx.acc_key] = _ROLLOUT_USES.get(ctx.acc_key, 0) + 1
            ctx.param_refs = (W1, b1, W2, b2, ln_w, ln_b)   # for .grad views only (DIRECT_PARAM_GRADS)
            # the node MLP of a factorised layer: its dense source-0 gradient is posted for the node-level product's backward
            ctx.mail_post = (MAIL_TOKEN if (_MAIL_POST and MAIL_TOKEN in _MAIL_CONSUMERS and geom.nsrc == 2 and geom.dmode[0] == 1 and geom.src_idx[0] is None
                                            and not geom.aggregate and ctx.needs_input_grad[7]) else None)
            if GRAD_LISTENER is not None:
                GRAD_LISTENER.note_use([q for q in ctx.param_refs if q is not None and q.requires_grad])
            ctx.save_for_backward(W1c, W2c, ln_w, z1, xhat, rstd, *[bi[0] for bi in binfo])
            ctx.set_materialize_grads(False)
        if out is not None:
            out = out.reshape(*lead, out.shape[-2], dout) if len(lead) != 1 else out
        if aggr is not None:
            aggr = aggr.reshape(*lead, geom.nseg_total, dout) if len(lead) != 1 else aggr
        return out, aggr

    @staticmethod
    def backward(ctx, g_out, g_aggr):
        return _fused_mlp_backward(ctx, g_out, g_aggr, ctx.needs_input_grad)


def _fused_mlp_backward(ctx, g_out, g_aggr, needs):
    """Backward of one fused-MLP launch (FusedMLPFunction / CatMLPFunction).  ``needs`` = the needs_input_grad tuple in
    FusedMLPFunction's argument order: (geom, W1, b1, W2, b2, ln_w, ln_b, *sources)."""
    lib = L.load()
    geom: MlpGeometry = ctx.geom
    W1, W2, ln_w, z1, xhat, rstd, *bases = ctx.saved_tensors
    B, rows, ntiles = ctx.B, ctx.rows, ctx.ntiles
    hid, kin = W1.shape
    dout = W2.shape[0]
    dev = W1.device
    nsrc = geom.nsrc
    widths = [s[-1] for s in ctx.src_shapes]
    n_fixed = 7
    # (a twin edge launch registered as mailbox consumer: whatever happens below, the post is taken out of the box)
    posted = _MAILBOX.pop(ctx.mail, None) if getattr(ctx, "mail", None) is not None else None
    if g_out is None and g_aggr is None:
        key_ = getattr(ctx, "acc_key", None)
        held = None
        if key_ is not None:   # nothing to add, but this consumer counts: the last one reports what the others collected
            _ROLLOUT_USES[key_] = _ROLLOUT_USES.get(key_, 1) - 1
            if _ROLLOUT_USES[key_] <= 0:
                held = _ROLLOUT_ACC.pop(key_, None)
        if held is not None:
            shape0 = ctx.src_shapes[0]
            return (None,) * n_fixed + (held.reshape(shape0) if held.numel() == math.prod(shape0) else held.sum(0).reshape(shape0),) + (None,) * (nsrc - 1)
        return (None,) * (n_fixed + nsrc)
    if g_out is not None:
        g_out = g_out.reshape(B, -1, dout).contiguous()
    if g_aggr is not None:
        g_aggr = g_aggr.reshape(B, -1, dout).contiguous()

    p = L.MlpBwd()
    for k in range(nsrc):
        b_, bstride = ctx.binfo[k]
        _fill_src(p.src[k], bases[k], bstride if b_ == B or B == 1 else 0, widths[k], geom.src_idx[k])
    p.nsrc, p.batch, p.rows, p.ntiles = nsrc, B, rows, ntiles
    p.tiles = _ptr(geom.tiles)
    p.W1, p.W2, p.ln_w = _ptr(W1), _ptr(W2), _ptr(ln_w) if ctx.has_ln else None
    p.hid, p.dout, p.flags, p.nseg_total = hid, dout, geom.flags | ctx.mm_flags, geom.nseg_total   # = rows of g_aggr per batch item
    nseg_rows = geom.nseg_ext if geom.comb is not None else geom.nseg_total   # rows of a receiver-gradient buffer (mode 3)
    pre = bool(geom.flags & L.F_PRE_ADD)
    p.ldw1 = kin if pre else 0
    if g_out is not None:
        p.g_out, p.out_idx, p.out_bstride = _ptr(g_out), _ptr(geom.out_idx), g_out.shape[1] * dout
    if g_aggr is not None:
        p.g_aggr, p.seg_of_row = _ptr(g_aggr), _ptr(geom.seg_of_row)
    p.rowptr, p.inv_deg = _ptr(geom.rowptr), _ptr(geom.inv_deg)
    p.z1, p.xhat, p.rstd = _ptr(z1), _ptr(xhat), _ptr(rstd)
    gemm = bool(getattr(ctx, "gemm", False))   # the forward ran on the tiled-GEMM family: so does the backward
    sbf = bool(getattr(ctx, "store_bf16", False))   # the forward saved z1 / xhat as bf16 rows: dz1 / dz2 leave as bf16 too
    if sbf:
        p.flags = int(p.flags) | L.F_STORE_BF16
    dz1 = torch.empty((B * rows, hid), device=dev, dtype=torch.bfloat16 if sbf else torch.float32)
    p.dz1 = _ptr(dz1)
    dsrc = [None] * nsrc
    tmp2 = [None] * nsrc
    for k in range(nsrc):
        if not needs[n_fixed + k]:
            p.dmode[k] = 0
            continue
        mode = geom.dmode[k]
        w = widths[k]
        n_src_rows = ctx.src_shapes[k][-2]
        p.dmode[k] = mode
        if pre and k > 0 and mode == 2:
            p.dmode[k] = 0   # gradient of a sender-gathered addend: a CSC segment sum over the dz1 rows, below
            continue
        if mode == 1:
            # rows scattered through the (unique, covering) gather index, or identity
            dsrc[k] = torch.empty((B, n_src_rows, w), device=dev, dtype=torch.float32)
            p.dsrc[k], p.dsrc_bstride[k] = _ptr(dsrc[k]), n_src_rows * w
        elif mode == 2:
            tmp2[k] = torch.empty((B, rows, w), device=dev, dtype=torch.float32)
            p.dsrc[k], p.dsrc_bstride[k] = _ptr(tmp2[k]), rows * w
        elif mode == 3:
            alloc = torch.zeros if geom.has_split else torch.empty
            dsrc[k] = alloc((B, nseg_rows, w), device=dev, dtype=torch.float32)
            p.dsrc[k], p.dsrc_bstride[k] = _ptr(dsrc[k]), nseg_rows * w
    if sbf or gemm:
        dz2, dpad = torch.empty((B * rows, dout), device=dev, dtype=torch.bfloat16 if sbf else torch.float32), dout
        p.dz2, p.dz2_ld = _ptr(dz2), 0
    else:
        dz2, dpad = _alloc_dz2(lib, p, B * rows, dout, dev)   # (rows, dout); 32-padded columns for a ragged output width (output_map)
    # Gradient hand-over across the autoregressive steps of a rollout (round 6): a static edge embedding is computed once per
    # rollout and is source 0 of one edge launch per AR step; every step's backward used to report its own (E, d) gradient and
    # autograd added them (0.1 - 0.5 GB per add at d = 512: 3.7 ms of the cfg5 step).  The first back-propagated step's buffer
    # is what autograd holds; the later ones add into it inside the kernel (NLAM_F_ACC_DSRC0) and report nothing.
    # Gradients are HELD BACK until the last of the tensor's consumers (counted in forward) is back-propagated, which reports the
    # sum: autograd sees one contribution from the fused launches, whatever else contributes to the tensor.
    acc_report = None   # set on the last consumer: what it reports for source 0
    acc_key = getattr(ctx, "acc_key", None)
    if acc_key is not None:
        remaining = _ROLLOUT_USES.get(acc_key, 1) - 1
        _ROLLOUT_USES[acc_key] = remaining
        prev = _ROLLOUT_ACC.get(acc_key)
        fam2 = (not gemm and dsrc[0] is not None and int(p.dmode[0]) == 1 and lib.nlam_mlp_bwd_family(C.byref(p)) == 2
                and (prev is None or prev.shape == dsrc[0].shape))
        if prev is None:
            if remaining > 0 and fam2:
                _ROLLOUT_ACC[acc_key] = dsrc[0]   # first of several: written by this launch, reported by the last
                acc_report, dsrc[0] = "held", None
        elif fam2:
            p.flags = int(p.flags) | L.F_ACC_DSRC0
            p.dsrc[0] = _ptr(prev)
            dsrc[0] = None
            ROLLOUT_ACC_STATS["accumulated"] += 1
            acc_report = prev if remaining <= 0 else "held"
        elif remaining <= 0 and dsrc[0] is not None:   # a launch of another kernel family closes the sequence: add what was held back
            acc_report = "flush"
        if remaining <= 0:
            _ROLLOUT_ACC.pop(acc_key, None)
            if acc_report == "flush":
                acc_report = prev
    nwp = 0 if gemm else lib.nlam_mlp_bwd_wpack_floats(C.byref(p))
    wpack = None
    if gemm:
        nws = _gemm_ws(lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(p)), "nlam_mlp_bwd_gemm_workspace_floats")
        wpack = torch.empty((max(nws, 1),), device=dev, dtype=torch.float32)
        p.wpack, p.wpack_floats = _ptr(wpack), nws
    elif nwp > 0:
        wpack = _wide_wpack(p, nwp, "b", ("b", W1.data_ptr(), W2.data_ptr(), tuple(widths), hid, dout, int(p.flags) & ~(L.F_STORE_BF16 | L.F_ACC_DSRC0), int(p.ldw1),
                                          rows, ntiles, B, tuple(int(p.dmode[k]) for k in range(nsrc)), int(p.dz2_ld)), dev, not geom.no_pack)
    elif ctx.pack is not None and PACKER is not None and ctx.pack.packed_step == PACKER.step_id:
        p.wpack, p.wpack_floats = ctx.pack.bwd.data_ptr(), ctx.pack.bwd.numel()
    nblk = lib.nlam_mlp_bwd_gemm_blocks(C.byref(p)) if gemm else lib.nlam_mlp_bwd_blocks(C.byref(p))
    vs = _vec_stride(hid, dout)
    vecp = torch.empty((nblk, 4, vs), device=dev, dtype=torch.float32)
    p.vec_partials, p.vec_partials_rows, p.vec_stride = _ptr(vecp), nblk, vs

    prm = ctx.param_refs
    pneeds = [needs[1], needs[2], needs[3], needs[4], ctx.has_ln and needs[5], ctx.has_ln and needs[6]]   # dW1, db1, dW2, db2, dgamma, dbeta
    on_side = OVERLAP.active and _all_direct(prm, pneeds)
    whole_side = on_side and not any(needs[n_fixed:])
    key = ("mlp_bwd", rows * B, kin, hid, dout, nsrc, g_aggr is not None)

    def bwd_meta():
        nbytes = sum(t_.numel() * t_.element_size() for t_ in (g_out, g_aggr, z1, xhat, rstd, dz1, dz2) if t_ is not None)
        nbytes += sum(t_.numel() * 4 for t_ in (*dsrc, *tmp2) if t_ is not None)
        # the minimum the math needs: incoming gradients once, data gradients once, and the cheaper of {the saved
        # tensors, the input rows a recomputing backward would gather instead}; dz1 / dz2 (they exist only because the weight
        # gradient is another launch) and the tile-row-order scratch of the sender gradient are not algorithmic
        saved = sum(t_.numel() * t_.element_size() for t_ in (z1, xhat, rstd) if t_ is not None)
        nmin = sum(t_.numel() * t_.element_size() for t_ in (g_out, g_aggr) if t_ is not None)
        nmin += sum(t_.numel() * 4 for t_ in dsrc if t_ is not None) + min(saved, rows * B * kin * 4)
        kin_live = sum(w_ for k_, w_ in enumerate(widths) if p.dmode[k_] != 0 and not (pre and k_ > 0))
        name, mf = _gemm_mm(ctx.mm_flags) if gemm else _mm_executed(ctx.mm_flags, hid, dout, [w_ for k_, w_ in enumerate(widths) if p.dmode[k_] != 0] or [hid],
                                                                     ragged_out_ok=dpad != dout)
        return {"flops": 2.0 * rows * B * (kin_live * hid + hid * dout), "bytes": float(nbytes), "bytes_min": float(nmin), "mm": name, "mfmas_per_block": mf,
                "what": "LayerNorm/SiLU backward + dh = dz2 W2 + dx = dz1 W1 (data gradients; writes dz1, dz2 for the weight gradients)"}

    bwd_fn = lib.nlam_mlp_bwd_gemm if gemm else lib.nlam_mlp_bwd

    def launch_data():
        L.check(PROFILE.launch(key, lambda: bwd_fn(C.byref(p), _stream()), bwd_meta), bwd_fn.__name__)

    if not whole_side:
        launch_data()
    if geom.comb is not None:   # receiver gradients of split receivers: sum their pieces, drop the virtual rows
        for k in range(nsrc):
            if dsrc[k] is not None and p.dmode[k] == 3:
                split_combine(dsrc[k], geom)
                dsrc[k] = dsrc[k][:, : geom.nseg_total]
                if B > 1:
                    dsrc[k] = dsrc[k].contiguous()

    if pre:
        for k in range(1, nsrc):
            if needs[n_fixed + k] and geom.dmode[k] == 2:   # no (rows, w) round trip: dz1 is the data
                if sbf:
                    dsrc[k] = torch.empty((B, geom.num_send, hid), device=dev, dtype=torch.float32)
                    L.check(lib.nlam_segment_sum_bf16(_ptr(dz1), rows * hid, _ptr(geom.colptr), _ptr(geom.cperm), None, _ptr(dsrc[k]),
                                                      geom.num_send, hid, B, _stream()), "nlam_segment_sum_bf16")
                else:
                    dsrc[k] = segment_sum(dz1, rows * hid, geom.colptr, geom.cperm, None, geom.num_send, hid, B)
    for k in range(nsrc):
        if tmp2[k] is not None:  # finish scatter-by-sender as a CSC segment sum
            tw = ctx.twin_of.get(k)
            if tw is not None and dsrc[tw] is not None and dsrc[tw].shape == (B, geom.num_send, widths[k]) and dsrc[tw].is_contiguous():
                # senders and receivers are the same tensor (mesh <-> mesh layers): add onto the receiver-side
                # gradient and report nothing for this slot -- one autograd add launch less per layer
                if posted is not None and posted.shape == dsrc[tw].shape and posted.is_contiguous():
                    # ... and both onto the gradient the layer's node MLP has already handed to autograd: nothing to report at all
                    L.check(lib.nlam_segment_sum_add(_ptr(tmp2[k]), rows * widths[k], _ptr(geom.colptr), _ptr(geom.cperm), None, _ptr(dsrc[tw]),
                                                     _ptr(posted), geom.num_send, widths[k], B, _stream()), "nlam_segment_sum_add")
                    MAIL_STATS["consumed"] += 1
                    dsrc[tw] = None
                    posted = None
                else:
                    segment_sum(tmp2[k], rows * widths[k], geom.colptr, geom.cperm, None, geom.num_send, widths[k], B,
                                out=dsrc[tw], accumulate=True)
                dsrc[k] = None
            else:
                dsrc[k] = segment_sum(
                    tmp2[k], rows * widths[k], geom.colptr, geom.cperm, None, geom.num_send, widths[k], B
                )

    tok = getattr(ctx, "mail_post", None)
    if tok is not None and dsrc[0] is not None and dsrc[0].is_contiguous():
        b0, _ = ctx.binfo[0]
        if b0 == B or B == 1:   # the source had its own batch dimension: dsrc[0] IS the gradient autograd receives
            _MAILBOX[tok] = dsrc[0]
            MAIL_STATS["posted"] += 1

    # ---- weight gradients: TN GEMMs with a deterministic two-stage reduction ----
    def wgrad(A, m, src_list, n, flags):
        q, partials = _wgrad_request(A, m, n, B, rows, src_list, flags | ctx.mm_flags | _wgrad_solo(), dev)
        key = ("wgrad", rows * B, m, n)

        def wg_meta():
            nsrc_b = sum(t.shape[-2] * w * t.element_size() * (B if bstride != 0 or B == 1 else 1) for (t, bstride, w, idx) in src_list)
            nbytes = A.numel() * A.element_size() + partials.numel() * 4 + nsrc_b
            nmin = A.numel() * A.element_size() + nsrc_b + m * n * 4   # operands once, dW once: partial sums are not algorithmic
            narrow = m <= 64 and all(w <= 64 for (_, _, w, _) in src_list)
            name, mf = ("f32", 0) if narrow else _mm_executed(ctx.mm_flags, m, m, [w for (_, _, w, _) in src_list])
            return {"flops": 2.0 * rows * B * m * n, "bytes": float(nbytes), "bytes_min": float(nmin), "mm": name, "mfmas_per_block": mf,
                    "what": "weight gradient dW = A^T [gathered B], rows = MFMA K"}

        L.check(PROFILE.launch(key, lambda: lib.nlam_wgrad(C.byref(q), _stream()), wg_meta), "nlam_wgrad")
        return partials

    src_list = []
    for k in range(1 if pre else nsrc):   # factorised: W1 has columns for source 0 only (the node-level products own the rest)
        b_, bstride = ctx.binfo[k]
        src_list.append((bases[k], bstride if b_ == B or B == 1 else 0, widths[k], geom.src_idx[k]))
    kin1 = widths[0] if pre else kin
    results = [None] * 6   # dW1, db1, dW2, db2, dgamma, dbeta

    def launch_weights():
        part1 = wgrad(dz1, hid, src_list, kin1, L.F_A_BF16 if sbf else 0) if needs[1] else None
        part2 = wgrad(dz2, dpad, [(z1, rows * hid, hid, None)], hid, L.F_SILU_B | ((L.F_A_BF16 | L.F_S_BF16) if sbf else 0)) if needs[3] else None
        # ---- one launch reduces every partial sum; with DIRECT_PARAM_GRADS it accumulates into .grad ----
        batch = _ReduceBatch(dev)
        results[:] = _mlp_reduce_jobs(batch, part1, part2, vecp, nblk, vs, 4, (hid, kin, dout), prm, pneeds, ctx.has_ln, ncols=kin1 if pre else 0)
        batch.flush()
        if on_side:
            OVERLAP.hold(torch.cuda.current_stream(), part1, part2)
        if GRAD_LISTENER is not None:   # inside the side-stream context: a collective launched from here waits on it
            GRAD_LISTENER.note_done([q for q, nd in zip(prm, pneeds) if nd and q is not None and _direct_grad(q, q.shape)])

    # Where the launches go: weight gradients (needed only by the optimizer) on a side stream when the trainer owns the
    # parameter gradients (see _WgradOverlap); an MLP none of whose inputs needs a gradient is a dead end of backward, so
    # its data-gradient kernel goes there as well.
    # Small weight gradients of the narrow family wait in WGRAD_BATCH for their like and leave together (grouped launches).  An
    # MLP that was deferred earlier in this step keeps the collector's stream for whatever else it launches: the accumulations
    # into its .grad stay ordered.
    side_owner, handed_over = prm[0], False
    if on_side and WGRAD_BATCH.enabled():
        req1 = (dz1, hid, kin1, src_list, ctx.mm_flags | _wgrad_solo())
        req2 = (dz2, dpad, hid, [(z1, rows * hid, hid, None)], L.F_SILU_B | ctx.mm_flags | _wgrad_solo())
        if (not whole_side and not sbf and needs[1] and needs[3] and id(prm[0]) not in OVERLAP.assigned
                and WGRAD_BATCH.wants(B, rows, req1, req2)):
            njobs = 2 + sum(1 for x in (pneeds[1], pneeds[3], ctx.has_ln and pneeds[4], ctx.has_ln and pneeds[5]) if x)
            WGRAD_BATCH.add(_WgradMember(prm[0], B, rows, (hid, kin, dout), req1, req2, vecp, nblk, vs, prm, pneeds, ctx.has_ln,
                                         kin1 if pre else 0, njobs))
            handed_over = True   # nothing is launched here
        elif id(prm[0]) in WGRAD_BATCH.seen:
            WGRAD_BATCH.flush()
            side_owner = WGRAD_BATCH
    if handed_over:
        pass
    elif whole_side:
        OVERLAP.run(side_owner, (g_out, g_aggr, xhat, rstd, wpack, dz1, dz2, vecp, z1, *bases), lambda: (launch_data(), launch_weights()), dead_end=True)
    elif on_side:
        OVERLAP.run(side_owner, (dz1, dz2, vecp, z1, *bases), launch_weights)
    else:
        launch_weights()
    dW1, db1, dW2, db2, dg, dbt = results

    if isinstance(acc_report, torch.Tensor):
        # the held-back sum: reported as it is when this launch accumulated into it, added to this launch's own gradient when it could not
        dsrc[0] = acc_report if dsrc[0] is None else dsrc[0].add_(acc_report)
    grads_src = [None if g is None else _unbatch_grad(g, ctx.src_shapes[k], B) for k, g in enumerate(dsrc)]
    return (None, dW1, db1, dW2, db2, dg, dbt, *grads_src)


@dataclass
class ChunkedGeometry:
    """Static description of a CHUNKED fused-MLP call site (``SplitMLPs``, gnn_layers.py:274-324: rows [r0, r1) of the
    input go through the chunk's own MLP).  Rows are in their original order; per source either the chunk's rows are
    a slice of the source tensor ("slice") or are gathered through an index ("gather")."""

    nsrc: int
    chunks: list                      # [(r0, r1), ...] covering 0 .. rows
    rows: int
    src_mode: list                    # "slice" | "gather" per source
    src_idx: list                     # gather: int32 (rows,) device tensor of source rows; slice: None
    flags_fwd: int = 0
    flags_bwd: int = 0
    # optional aggregation of the output rows onto receivers (CSR over all rows)
    rowptr: torch.Tensor | None = None
    perm: torch.Tensor | None = None
    inv_deg: torch.Tensor | None = None
    seg_of_row: torch.Tensor | None = None
    num_rec: int = 0
    mean: bool = False
    # per gathered source: (ptr, order, nseg) of the segment sum that turns per-row gradients into per-source-row ones
    scatter: list = field(default_factory=lambda: [None, None, None])


def _row_window(x: torch.Tensor):
    """(..., N, w) -> (tensor to keep alive, B, batch stride in floats): no copy for contiguous tensors and stride-0 batches."""
    t, B, bstride, _ = as_batched(x)
    return t, B, bstride


def _chunk_sources(geom, bases, win_meta, widths, B, r0):
    """The sources of the chunk that starts at row ``r0``, as (address, batch stride, width, index address | None) per source
    (``win_meta``: (B, batch stride) of each, _row_window): what its launches and its weight-gradient request read."""
    srcs = []
    for k in range(geom.nsrc):
        b_, bstride = win_meta[k]
        bs = bstride if (b_ == B or B == 1) else 0
        if geom.src_mode[k] == "slice":
            srcs.append((bases[k].data_ptr() + 4 * r0 * widths[k], bs, widths[k], None))
        else:
            srcs.append((bases[k].data_ptr(), bs, widths[k], geom.src_idx[k].data_ptr() + 4 * r0))
    return srcs


class ChunkedMLPFunction(torch.autograd.Function):
    """``SplitMLPs`` (gnn_layers.py:274-324) inside an InteractionNet, natively: every chunk is one launch of the fused
    kernels on its row window of shared input / output buffers (no torch.split / cat copies, no index_select), the
    aggregation is one CSR segment sum, and in backward the gradients of gathered sources are finished by one
    segment sum per source over all chunks -- fixed summation orders throughout (the reference trains with
    ``deterministic=True``, train_model.py:566).

    forward(geom, nchunks, [W1, b1, W2, b2, ln_w, ln_b] * nchunks, *sources) -> (out (B, rows, dout), aggr | None)
    """

    @staticmethod
    def forward(ctx, geom: ChunkedGeometry, nchunks: int, *flat):
        lib = L.load()
        params = [flat[6 * c : 6 * c + 6] for c in range(nchunks)]
        srcs = flat[6 * nchunks :]
        assert len(srcs) == geom.nsrc and len(geom.chunks) == nchunks
        mm_flags = _mm_flags()
        srcs = tuple(s if s.dtype == torch.float32 else s.float() for s in srcs)
        _require_gpu(*[q for pr in params for q in pr], *srcs)
        win = [_row_window(s) for s in srcs]
        B = max(w[1] for w in win)
        widths = [s.shape[-1] for s in srcs]
        nrows_src = [s.shape[-2] for s in srcs]
        hid, kin = params[0][0].shape
        dout = params[0][2].shape[0]
        if sum(widths) != kin:
            raise RuntimeError(f"source widths {widths} do not add up to the first Linear's in_features {kin}")
        dev = srcs[0].device
        R = geom.rows
        need_grad = any(ctx.needs_input_grad[2:])
        has_ln = params[0][4] is not None
        out = torch.empty((B, R, dout), device=dev, dtype=torch.float32)
        saved = []
        keep = []
        launches = []
        for c, (r0, r1) in enumerate(geom.chunks):
            W1, b1, W2, b2, ln_w, ln_b = params[c]
            rows = r1 - r0
            if rows == 0:
                saved.append((None, None, None))
                continue
            p = L.MlpFwd()
            for k, src in enumerate(_chunk_sources(geom, [w[0] for w in win], [w[1:] for w in win], widths, B, r0)):
                _fill_src(p.src[k], *src)
            p.nsrc, p.batch, p.rows, p.ntiles = geom.nsrc, B, rows, (rows + 31) // 32
            W1c, b1c, W2c, b2c = W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()
            keep.extend((W1c, b1c, W2c, b2c))
            p.W1, p.b1, p.W2, p.b2, p.ln_w, p.ln_b = _ptr(W1c), _ptr(b1c), _ptr(W2c), _ptr(b2c), _ptr(ln_w), _ptr(ln_b)
            p.eps, p.hid, p.dout, p.flags = 1e-5, hid, dout, geom.flags_fwd | mm_flags
            p.out, p.out_bstride = out.data_ptr() + 4 * r0 * dout, R * dout
            z1 = xhat = rstd = None
            if need_grad:
                z1 = torch.empty((B, rows, hid), device=dev, dtype=torch.float32)
                p.z1 = _ptr(z1)
                if has_ln:
                    xhat = torch.empty((B, rows, dout), device=dev, dtype=torch.float32)
                    rstd = torch.empty((B, rows), device=dev, dtype=torch.float32)
                    p.xhat, p.rstd = _ptr(xhat), _ptr(rstd)
            nwp = lib.nlam_mlp_fwd_wpack_floats(C.byref(p))
            if nwp > 0:
                # (under a trainer: packed once per step with every other wide MLP of the model, nlam_pack_records)
                keep.append(_wide_wpack(p, nwp, "f", ("cf", W1c.data_ptr(), W2c.data_ptr(), tuple(widths), hid, dout, int(p.flags), rows, B), dev))
            launches.append(p)
            saved.append((z1, xhat, rstd))
        _launch_chunks(lib, "fwd", launches)
        aggr = None
        if geom.rowptr is not None:
            aggr = segment_sum(out, R * dout, geom.rowptr, geom.perm, geom.inv_deg if geom.mean else None, geom.num_rec, dout, B)
        if need_grad:
            ctx.geom, ctx.B, ctx.nchunks, ctx.mm_flags, ctx.has_ln = geom, B, nchunks, mm_flags, has_ln
            ctx.win_meta = [(w[1], w[2]) for w in win]
            ctx.src_shapes = [tuple(s.shape) for s in srcs]
            ctx.params = params
            ctx.saved_acts = saved
            ctx.bases = [w[0] for w in win]
            ctx.set_materialize_grads(False)
            if GRAD_LISTENER is not None:
                GRAD_LISTENER.note_use([q for pr in params for q in pr if q is not None and q.requires_grad])
        lead = max((tuple(s.shape[:-2]) for s in srcs), key=len)
        if len(lead) != 1:
            out = out.reshape(*lead, R, dout)
            aggr = aggr.reshape(*lead, geom.num_rec, dout) if aggr is not None else None
        return out, aggr

    @staticmethod
    def backward(ctx, g_out, g_aggr):
        lib = L.load()
        geom: ChunkedGeometry = ctx.geom
        B, nchunks = ctx.B, ctx.nchunks
        nsrc = geom.nsrc
        n_fixed = 2 + 6 * nchunks
        if g_out is None and g_aggr is None:
            return (None,) * (n_fixed + nsrc)
        params = ctx.params
        hid, kin = params[0][0].shape
        dout = params[0][2].shape[0]
        widths = [s[-1] for s in ctx.src_shapes]
        nrows_src = [s[-2] for s in ctx.src_shapes]
        dev = params[0][0].device
        R = geom.rows
        if g_out is not None:
            g_out = g_out.reshape(B, R, dout).contiguous()
        if g_aggr is not None:
            g_aggr = g_aggr.reshape(B, geom.num_rec, dout).contiguous()
        need_src = [ctx.needs_input_grad[n_fixed + k] for k in range(nsrc)]
        # gradient buffers: sliced sources get their rows written in place; gathered ones a (B, R, w) row-order buffer
        dbuf = [None] * nsrc
        for k in range(nsrc):
            if need_src[k]:
                nr = nrows_src[k] if geom.src_mode[k] == "slice" else R
                dbuf[k] = torch.empty((B, nr, widths[k]), device=dev, dtype=torch.float32)
        tmp_chunks = [[] for _ in range(nsrc)]   # B > 1: per-chunk (B, rows_c, w) buffers of gathered sources
        launches, work = [], []
        for c, (r0, r1) in enumerate(geom.chunks):
            W1, b1, W2, b2, ln_w, ln_b = params[c]
            rows = r1 - r0
            needs = [ctx.needs_input_grad[2 + 6 * c + q] for q in range(6)]
            if rows == 0:
                continue
            z1, xhat, rstd = ctx.saved_acts[c]
            W1c, W2c = W1.contiguous(), W2.contiguous()
            p = L.MlpBwd()
            src_list = _chunk_sources(geom, ctx.bases, ctx.win_meta, widths, B, r0)
            for k, src in enumerate(src_list):
                _fill_src(p.src[k], *src)
            p.nsrc, p.batch, p.rows, p.ntiles = nsrc, B, rows, (rows + 31) // 32
            p.W1, p.W2, p.ln_w = _ptr(W1c), _ptr(W2c), _ptr(ln_w) if ctx.has_ln else None
            p.hid, p.dout, p.flags, p.nseg_total = hid, dout, geom.flags_bwd | ctx.mm_flags, geom.num_rec
            if g_out is not None:
                p.g_out, p.out_bstride = g_out.data_ptr() + 4 * r0 * dout, R * dout
            if g_aggr is not None:
                p.g_aggr, p.seg_of_row = _ptr(g_aggr), geom.seg_of_row.data_ptr() + 4 * r0
                p.inv_deg = _ptr(geom.inv_deg)
            p.z1, p.xhat, p.rstd = _ptr(z1), _ptr(xhat), _ptr(rstd)
            dz1 = torch.empty((B * rows, hid), device=dev, dtype=torch.float32)
            p.dz1 = _ptr(dz1)
            for k in range(nsrc):
                if not need_src[k]:
                    p.dmode[k] = 0
                elif geom.src_mode[k] == "slice":
                    p.dmode[k] = 1
                    p.dsrc[k], p.dsrc_bstride[k] = dbuf[k].data_ptr() + 4 * r0 * widths[k], nrows_src[k] * widths[k]
                else:
                    p.dmode[k] = 2
                    if B == 1:
                        p.dsrc[k], p.dsrc_bstride[k] = dbuf[k].data_ptr() + 4 * r0 * widths[k], rows * widths[k]
                    else:
                        tc = torch.empty((B, rows, widths[k]), device=dev, dtype=torch.float32)
                        tmp_chunks[k].append(tc)
                        p.dsrc[k], p.dsrc_bstride[k] = _ptr(tc), rows * widths[k]
            dz2, dpad = _alloc_dz2(lib, p, B * rows, dout, dev)
            nwp = lib.nlam_mlp_bwd_wpack_floats(C.byref(p))
            wpack = None
            if nwp > 0:
                wpack = _wide_wpack(p, nwp, "b", ("cb", W1c.data_ptr(), W2c.data_ptr(), tuple(widths), hid, dout, int(p.flags), rows, B,
                                                  tuple(int(p.dmode[k]) for k in range(nsrc)), int(p.dz2_ld)), dev)
            nblk = lib.nlam_mlp_bwd_blocks(C.byref(p))
            vs = _vec_stride(hid, dout)
            vecp = torch.empty((nblk, 4, vs), device=dev, dtype=torch.float32)
            p.vec_partials, p.vec_partials_rows, p.vec_stride = _ptr(vecp), nblk, vs
            launches.append(p)
            work.append((c, src_list, rows, z1, dz1, dz2, vecp, vs, needs, (wpack, W1c, W2c)))
        # data gradients: the chunks of the fp32 wide family in one grid, the others one launch each; `nblks` = the rows of
        # vec_partials every launch wrote
        nblks = _launch_chunks(lib, "bwd", launches)
        # ---- weight gradients per chunk (deterministic two-stage reductions).  Under a trainer they leave the chain: the
        # optimizer is their only reader, and in one stream they were 2/3 of a chunk's backward chain.  ALL chunks go to ONE
        # side stream in ONE fork: forked one by one, the seven forks of an edge stage are edges 0 .. 6 of the same chain kernel,
        # the chain's next kernel is edge 7, and the graph executor (DESIGN finding 38) puts it on a hardware queue behind one
        # chunk's weight gradients -- 150 us of waiting per processor layer in the replayed cfg4p step ----
        done = {}
        side, here = [], []
        for (c, src_list, rows, z1, dz1, dz2, vecp, vs, needs, _alive), nblk in zip(work, nblks):
            item = _WgradItem(B, rows, hid, dout, kin, ctx.mm_flags, dz1, dz2, z1, vecp, nblk, vs, src_list, params[c], needs, ctx.has_ln)
            if OVERLAP.active and DIRECT_PARAM_GRADS and _all_direct(params[c], needs):   # (every gradient lands in the flat views: nothing to return)
                side.append(item)
                done[c] = [None] * 6
            else:
                here.append((c, item))
        for (c, _), res in zip(here, _chunks_weight_grads([it for _, it in here]) if here else []):
            done[c] = res
        grads_params = []
        for c, (r0, r1) in enumerate(geom.chunks):
            if c in done:
                grads_params.extend(done[c])
            else:   # an empty chunk
                needs = [ctx.needs_input_grad[2 + 6 * c + q] for q in range(6)]
                grads_params.extend([torch.zeros_like(q) if (q is not None and nd) else None for q, nd in zip(params[c], needs)])
        # ---- finish the gathered sources: one segment sum over all chunks' rows ----
        grads_src = []
        for k in range(nsrc):
            g = None
            if need_src[k]:
                if geom.src_mode[k] == "slice":
                    g = dbuf[k]
                else:
                    rowbuf = dbuf[k] if B == 1 else torch.cat(tmp_chunks[k], dim=1)
                    ptr, order, nseg = geom.scatter[k]
                    g = segment_sum(rowbuf, R * widths[k], ptr, order, None, nseg, widths[k], B)
                g = _unbatch_grad(g, ctx.src_shapes[k], B)
            grads_src.append(g)
        if side:   # forked behind the segment sums: those are the chain, and the fork takes their hardware queue (finding 38)
            OVERLAP.run(side[0].params[0], tuple(t for it in side for t in (it.dz1, it.dz2, it.vecp, it.z1)) + tuple(ctx.bases),
                        lambda: _chunks_weight_grads(side))
        return (None, None, *grads_params, *grads_src)


# chunks of the fp32 wide family (d = 128 below the super-tile threshold) share one grid per direction
GROUP_CHUNKS = os.environ.get("NLAM_GROUP_CHUNKS", "1") == "1"


def _launch_chunks(lib, which, launches):
    """Launch the fused kernels of a chunked MLP (``launches``: filled MlpFwd / MlpBwd structs): members of the fp32 wide
    family go <= NLAM_MAX_GROUP at a time into ONE grid (nlam_mlp_*_group; every other chunk of hi_lam_parallel.py:127-143
    at d = 128 is 3 .. 206 tiles -- a launch apiece leaves most of the chip idle for one tile's latency), the others one
    launch each.  Returns, per launch, the rows of ``vec_partials`` it wrote (backward; None forward)."""
    fwd = which == "fwd"
    family = lib.nlam_mlp_fwd_family if fwd else lib.nlam_mlp_bwd_family
    single = lib.nlam_mlp_fwd if fwd else lib.nlam_mlp_bwd
    group = lib.nlam_mlp_fwd_group if fwd else lib.nlam_mlp_bwd_group
    typ = L.MlpFwd if fwd else L.MlpBwd
    nblks = [None if fwd else int(p.vec_partials_rows) for p in launches]
    wide = [i for i, p in enumerate(launches) if GROUP_CHUNKS and int(family(C.byref(p))) == 1]
    grouped = set()
    for g0 in range(0, len(wide), L.NLAM_MAX_GROUP):
        members = wide[g0 : g0 + L.NLAM_MAX_GROUP]
        if len(members) < 2:
            continue
        m = len(members)
        arr = (typ * m)(*[launches[i] for i in members])
        if not fwd:
            blocks = (C.c_int32 * m)()
            L.check(lib.nlam_mlp_bwd_group_blocks(arr, m, blocks), "nlam_mlp_bwd_group_blocks")
            for j, i in enumerate(members):
                nblks[i] = int(blocks[j])
        rows_all = sum(int(arr[j].rows) * int(arr[j].batch) for j in range(m))
        rc = PROFILE.launch((f"mlp_{which}_group_wide", rows_all, m, int(arr[0].hid), int(arr[0].dout)), lambda: group(arr, m, _stream()))
        L.check(rc, f"nlam_mlp_{which}_group (chunks)")
        grouped.update(members)
    for i, p in enumerate(launches):
        if i not in grouped:
            L.check(single(C.byref(p), _stream()), f"nlam_mlp_{which} (chunk)")
    return nblks


GROUP_WGRADS = os.environ.get("NLAM_GROUP_WGRADS", "1") == "1"


def _chunks_weight_grads(items):
    """dW1, db1, dW2, db2, dgamma, dbeta of several fused MLPs from their saved row gradients (``items``: _WgradItem; the chunks
    of a ``SplitMLPs`` layer, gnn_layers.py:311-324, or one member of a grouped launch): every dW1 GEMM of one shape in ONE launch,
    every dW2 GEMM in one (``nlam_wgrad_group``: members of the split-bf16 wide family; others one launch each), and the
    reductions of up to NLAM_MAX_REDUCE_JOBS partial sums per launch -- 4 launches instead of 21 for the seven edge chunks of a
    Hi-LAM-Parallel layer.  Per member the arithmetic is that of its own launch: the results are bit-identical.  Returns one
    6-list per item (None where, in a trainer's direct-gradient mode, the sum landed in the flat gradient view)."""
    lib = L.load()
    dev = items[0].dz1.device

    def launch(qs):
        """members of one shape share a grid, NLAM_MAX_GROUP at a time"""
        classes = {}
        for q in qs:
            key = (int(q.m), int(q.n), int(q.nsrc), int(q.flags), tuple(int(q.src[k].width) for k in range(int(q.nsrc))))
            classes.setdefault(key, []).append(q)
        for members in classes.values():
            for g0 in range(0, len(members), L.NLAM_MAX_GROUP):
                grp = members[g0 : g0 + L.NLAM_MAX_GROUP]
                rc = -2
                if GROUP_WGRADS and len(grp) > 1:
                    arr = (L.Wgrad * len(grp))(*grp)
                    rows_all = sum(int(q.rows) * int(q.batch) for q in grp)
                    rc = PROFILE.launch(("wgrad_group", rows_all, len(grp), int(grp[0].m), int(grp[0].n)), lambda: lib.nlam_wgrad_group(arr, len(grp), _stream()))
                if rc == -2:
                    for q in grp:
                        L.check(lib.nlam_wgrad(C.byref(q), _stream()), "nlam_wgrad (chunk)")
                else:
                    L.check(rc, "nlam_wgrad_group")

    parts = []
    q1s, q2s = [], []
    for it in items:
        part1 = part2 = None
        if it.needs[0]:
            q, part1 = _wgrad_request(it.dz1, it.hid, it.kin, it.B, it.rows, it.src_list, it.mm_flags, dev)
            q1s.append(q)
        if it.needs[2]:   # dz2 is (rows, dout), or 32-padded (zero columns) for a ragged output width: the first dout rows of the partials count
            q, part2 = _wgrad_request(it.dz2, it.dz2.shape[1], it.hid, it.B, it.rows, [(it.z1, it.rows * it.hid, it.hid, None)], L.F_SILU_B | it.mm_flags, dev)
            q2s.append(q)
        parts.append((part1, part2))
    launch(q1s)
    launch(q2s)

    all_results, done = [], []
    batch = _ReduceBatch(dev)
    for it, (part1, part2) in zip(items, parts):
        batch.reserve(6)
        all_results.append(_mlp_reduce_jobs(batch, part1, part2, it.vecp, it.nblk, it.vs, 4, (it.hid, it.kin, it.dout), it.params, it.needs, it.has_ln))
        done.extend(q for q, nd in zip(it.params, it.needs) if nd and q is not None and _direct_grad(q, q.shape))
    batch.flush()
    if GRAD_LISTENER is not None:
        GRAD_LISTENER.note_done(done)
    return all_results


def _alloc_dz2(lib, p, nrows, dout, dev):
    """The dz2 buffer of a backward launch (the row gradients of the second Linear, read by its weight gradient) with the row
    stride the kernel chosen for ``p`` writes: dout, or 32-padded with zero columns for a ragged output width on the
    split-bf16 kernels (``nlam_mlp_bwd_dz2_ld``).  Call once every field of ``p`` that decides the kernel is set."""
    ld = int(lib.nlam_mlp_bwd_dz2_ld(C.byref(p)))
    dpad = ld if ld > 0 else dout
    # the wide kernels write the real columns only: the padding must read as zeros in the weight gradient
    alloc = torch.zeros if (ld > 0 and lib.nlam_mlp_bwd_wpack_floats(C.byref(p)) > 0) else torch.empty
    dz2 = alloc((nrows, dpad), device=dev, dtype=torch.float32)
    p.dz2, p.dz2_ld = _ptr(dz2), ld
    return dz2, dpad


def _set_bwd_pack(p, pack):
    """Hand a narrow backward launch the weight image packed for this step (None / stale: the kernel stages its weights itself)."""
    if pack is not None and PACKER is not None and pack.packed_step == PACKER.step_id:
        p.wpack, p.wpack_floats = pack.bwd.data_ptr(), pack.bwd.numel()


# Leaf MLPs of <= 3 input columns accumulate their weight gradients inside the grouped backward kernel (NLAM_F_LEAF_WGRAD)
FUSED_LEAF_WGRAD = os.environ.get("NLAM_FUSED_LEAF_WGRAD", "1") == "1"


class GroupedMLPFunction(torch.autograd.Function):
    """n <= 8 independent single-source fused MLPs of one shape -- the embedders of the static grid / mesh / edge features
    (graph/base.py:286-295, hierarchical.py:195-231) -- in ONE launch each way (nlam_mlp_fwd_group / nlam_mlp_bwd_group):
    as separate launches each is a latency-bound link of the step's critical chain (4 x 14-50 us forward and 4 x 21-86 us
    at the very end of backward at cfg2).  Their inputs are data (no input gradients).  Shapes the grouped kernels do not
    cover run as a loop of single launches inside the same Function.

    forward(n, [W1, b1, W2, b2, ln_w, ln_b] * n, *xs) -> n outputs."""

    @staticmethod
    def forward(ctx, n: int, *flat):
        lib = L.load()
        params = [flat[6 * k : 6 * k + 6] for k in range(n)]
        xs = flat[6 * n :]
        assert len(xs) == n
        mm_flags = _mm_flags()
        xs = tuple(x if x.dtype == torch.float32 else x.float() for x in xs)
        _require_gpu(*[q for pr in params for q in pr], *xs)
        need_grad = any(ctx.needs_input_grad[1 : 1 + 6 * n])
        dev = xs[0].device
        arr = (L.MlpFwd * n)()
        outs, saved, keep, packs = [], [], [], []
        # leaf MLPs of <= 3 input columns: the grouped backward accumulates the weight gradients itself and recomputes the
        # pre-activation from the input (three FMAs per element), so the forward does not save z1 (a third of its bytes)
        lw = (n > 1 and FUSED_LEAF_WGRAD and (mm_flags >> 8) & 3 != 0
              and all(pr[0].shape[1] <= 3 and pr[0].shape[0] in (32, 64) and pr[2].shape[0] == pr[0].shape[0] for pr in params)
              and len({(pr[0].shape[0], pr[4] is None) for pr in params}) == 1 and all(x.dim() == 2 for x in xs))
        # ONE set of backward matrix-mode bits for the whole group (the kernel flags of the grouped backward launch and every
        # member's backward weight image must agree on the term count): narrow rules only when every member is narrow
        grp_bflags = _bwd_flags(mm_flags, all(max(*q[0].shape, q[2].shape[0]) <= 64 for q in params))
        for k in range(n):
            W1, b1, W2, b2, ln_w, ln_b = params[k]
            x = xs[k]
            t, B, bstride, lead = as_batched(x)
            rows, kin = x.shape[-2], x.shape[-1]
            hid, dout = W1.shape[0], W2.shape[0]
            if W1.shape[1] != kin:
                raise RuntimeError(f"grouped MLP {k}: input width {kin} does not match the first Linear {tuple(W1.shape)}")
            p = arr[k]
            _fill_src(p.src[0], t, bstride, kin, None)
            p.nsrc, p.batch, p.rows, p.ntiles = 1, B, rows, (rows + 31) // 32
            W1c, b1c, W2c, b2c = W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()
            keep.extend((t, W1c, b1c, W2c, b2c))
            p.W1, p.b1, p.W2, p.b2, p.ln_w, p.ln_b = _ptr(W1c), _ptr(b1c), _ptr(W2c), _ptr(b2c), _ptr(ln_w), _ptr(ln_b)
            p.eps, p.hid, p.dout, p.flags = 1e-5, hid, dout, mm_flags
            pack = None
            if PACKER is not None and max(hid, dout, kin) <= 64:
                pack = PACKER.get(W1c, W2c, [kin], hid, dout, False, 0, mm_flags)
                if pack is not None:
                    p.wpack, p.wpack_floats = pack.fwd.data_ptr(), pack.fwd.numel()
                pack = _bwd_pack(pack, mm_flags, grp_bflags, W1c, W2c, [kin], hid, dout, False, 0)
            packs.append(pack)
            out = torch.empty((B, rows, dout), device=dev, dtype=torch.float32)
            p.out, p.out_bstride = _ptr(out), rows * dout
            z1 = xhat = rstd = None
            if need_grad:
                if not lw:
                    z1 = torch.empty((B, rows, hid), device=dev, dtype=torch.float32)
                    p.z1 = _ptr(z1)
                if ln_w is not None:
                    xhat = torch.empty((B, rows, dout), device=dev, dtype=torch.float32)
                    rstd = torch.empty((B, rows), device=dev, dtype=torch.float32)
                    p.xhat, p.rstd = _ptr(xhat), _ptr(rstd)
            outs.append(out.reshape(*lead, rows, dout) if len(lead) != 1 else out)
            saved.append((t, B, bstride, rows, W1c, W2c, z1, xhat, rstd))
        rows_all = sum(int(arr[k].rows) * int(arr[k].batch) for k in range(n))

        def grp_meta():
            fl = sum(2.0 * arr[k].rows * arr[k].batch * (xs[k].shape[-1] * arr[k].hid + arr[k].hid * arr[k].dout) for k in range(n))
            by = sum(4.0 * arr[k].rows * arr[k].batch * (xs[k].shape[-1] + arr[k].dout + (arr[k].hid + arr[k].dout + 1 if need_grad else 0)) for k in range(n))
            name, mf = _mm_executed(mm_flags, arr[0].hid, arr[0].dout, [32])
            return {"flops": fl, "bytes": by, "mm": name, "mfmas_per_block": mf, "what": f"{n} static-feature embedders in one grouped launch"}

        fams = {int(lib.nlam_mlp_fwd_family(C.byref(arr[k]))) for k in range(n)}
        for k in range(n):   # wide members: the weights in MFMA A-operand order (packed once per step under a trainer)
            p = arr[k]
            nwp = lib.nlam_mlp_fwd_wpack_floats(C.byref(p))
            if nwp > 0:
                W1c, W2c = saved[k][4], saved[k][5]
                keep.append(_wide_wpack(p, nwp, "f", ("gf", W1c.data_ptr(), W2c.data_ptr(), int(p.src[0].width), int(p.hid), int(p.dout), int(p.flags),
                                                      int(p.rows), int(p.batch)), dev))
                packs[k] = None
        # one grid for members of the narrow family, or of the fp32 wide one (the embedders at d = 128); mixed families and
        # split-bf16 super-tile members run one launch each
        rc = PROFILE.launch(("mlp_fwd_group", rows_all, n, int(arr[0].hid), int(arr[0].dout)),
                            lambda: lib.nlam_mlp_fwd_group(arr, n, _stream()), grp_meta) if (n > 1 and fams in ({0}, {1})) else -2
        if rc == -2:   # NLAM_EUNSUP: members of different kernel shapes -> one launch each
            for k in range(n):
                L.check(lib.nlam_mlp_fwd(C.byref(arr[k]), _stream()), "nlam_mlp_fwd (group member)")
        else:
            L.check(rc, "nlam_mlp_fwd_group")
        if need_grad:
            ctx.lw = lw
            ctx.packs = packs
            ctx.n, ctx.params, ctx.saved, ctx.mm_flags = n, params, saved, grp_bflags
            ctx.set_materialize_grads(False)
            if GRAD_LISTENER is not None:
                GRAD_LISTENER.note_use([q for pr in params for q in pr if q is not None and q.requires_grad])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        lib = L.load()
        n, params = ctx.n, ctx.params
        dev = params[0][0].device
        live = [k for k in range(n) if g_outs[k] is not None]
        grads = [None] * (6 * n)
        if not live:
            return (None, *grads, *([None] * n))
        m = len(live)
        if ctx.lw:   # decided in forward (which did not save z1): the fused-weight-gradient kernel, for one or several live members
            if not _grouped_backward_fused(ctx, g_outs, live, grads):
                raise RuntimeError("nlam_mlp_bwd_group has no fused-weight-gradient kernel for a shape the forward planned it for")
            return (None, *grads, *([None] * n))
        arr = (L.MlpBwd * m)()
        work = []
        for i, k in enumerate(live):
            t, B, bstride, rows, W1c, W2c, z1, xhat, rstd = ctx.saved[k]
            hid, kin = W1c.shape
            dout = W2c.shape[0]
            g = g_outs[k].reshape(B, rows, dout).contiguous()
            p = arr[i]
            _fill_src(p.src[0], t, bstride, kin, None)
            p.nsrc, p.batch, p.rows, p.ntiles = 1, B, rows, (rows + 31) // 32
            p.W1, p.W2, p.ln_w = _ptr(W1c), _ptr(W2c), _ptr(params[k][4])
            p.hid, p.dout, p.flags = hid, dout, ctx.mm_flags
            p.g_out, p.out_bstride = _ptr(g), rows * dout
            p.z1, p.xhat, p.rstd = _ptr(z1), _ptr(xhat), _ptr(rstd)
            _set_bwd_pack(p, ctx.packs[k])
            dz1 = torch.empty((B * rows, hid), device=dev, dtype=torch.float32)
            p.dz1 = _ptr(dz1)
            dz2, _ = _alloc_dz2(lib, p, B * rows, dout, dev)
            work.append([k, g, dz1, dz2, None, 0, None])
        fams = {int(lib.nlam_mlp_bwd_family(C.byref(arr[i]))) for i in range(m)}
        for i, k in enumerate(live):   # wide members: transposed weights in MFMA A-operand order
            p = arr[i]
            nwp = lib.nlam_mlp_bwd_wpack_floats(C.byref(p))
            if nwp > 0:
                W1c, W2c = ctx.saved[k][4], ctx.saved[k][5]
                work[i][6] = _wide_wpack(p, nwp, "b", ("gb", W1c.data_ptr(), W2c.data_ptr(), int(p.src[0].width), int(p.hid), int(p.dout), int(p.flags),
                                                       int(p.rows), int(p.batch), int(p.dz2_ld)), dev)
        blocks = (C.c_int32 * m)()
        can_group = m > 1 and fams in ({0}, {1})
        if can_group:
            rcb = lib.nlam_mlp_bwd_group_blocks(arr, m, blocks)
            if rcb == -2:
                can_group = False
            else:
                L.check(rcb, "nlam_mlp_bwd_group_blocks")
        for i, k in enumerate(live):
            p = arr[i]
            hid, dout = p.hid, p.dout
            nblk_single = lib.nlam_mlp_bwd_blocks(C.byref(p))
            vs = _vec_stride(hid, dout)
            rows_v = max(int(blocks[i]), int(nblk_single))
            vecp = torch.empty((rows_v, 4, vs), device=dev, dtype=torch.float32)
            p.vec_partials, p.vec_partials_rows, p.vec_stride = _ptr(vecp), rows_v, vs
            work[i][4], work[i][5] = vecp, int(blocks[i])
        rows_all = sum(int(arr[i].rows) * int(arr[i].batch) for i in range(m))

        def grp_meta():
            fl = sum(2.0 * arr[i].rows * arr[i].batch * arr[i].hid * arr[i].dout for i in range(m))
            by = sum(4.0 * arr[i].rows * arr[i].batch * (3 * arr[i].dout + 2 * arr[i].hid + 1) for i in range(m))
            name, mf = _mm_executed(ctx.mm_flags, arr[0].hid, arr[0].dout, [32])
            return {"flops": fl, "bytes": by, "mm": name, "mfmas_per_block": mf,
                    "what": f"backward of {m} static-feature embedders in one grouped launch (no data gradients; writes dz1, dz2)"}

        rc = PROFILE.launch(("mlp_bwd_group", rows_all, m, int(arr[0].hid), int(arr[0].dout)),
                            lambda: lib.nlam_mlp_bwd_group(arr, m, _stream()), grp_meta) if can_group else -2
        if rc == -2:
            for i in range(m):
                p = arr[i]
                work[i][5] = lib.nlam_mlp_bwd_blocks(C.byref(p))
                L.check(lib.nlam_mlp_bwd(C.byref(p), _stream()), "nlam_mlp_bwd (group member)")
        else:
            L.check(rc, "nlam_mlp_bwd_group")
        # ---- weight gradients per member (side streams under the trainer) ----
        for i, k in enumerate(live):
            _, g, dz1, dz2, vecp, nblk, wpack = work[i]
            t, B, bstride, rows, W1c, W2c, z1, xhat, rstd = ctx.saved[k]
            hid, kin = W1c.shape
            dout = W2c.shape[0]
            prm = params[k]
            needs = [ctx.needs_input_grad[1 + 6 * k + q] for q in range(6)]
            has_ln = prm[4] is not None
            item = _WgradItem(B, rows, hid, dout, kin, ctx.mm_flags, dz1, dz2, z1, vecp, nblk, _vec_stride(hid, dout), [(t, bstride, kin, None)], prm, needs, has_ln)
            if OVERLAP.active and DIRECT_PARAM_GRADS and _all_direct(prm, needs):
                OVERLAP.run(prm[0], (g, dz1, dz2, vecp, z1, t, wpack), lambda it=item: _chunks_weight_grads([it]))
            else:
                grads[6 * k : 6 * k + 6] = _chunks_weight_grads([item])[0]
        return (None, *grads, *([None] * n))


def _grouped_backward_fused(ctx, g_outs, live, grads):
    """Grouped backward with the weight gradients accumulated in the kernel (NLAM_F_LEAF_WGRAD): one launch produces, per
    member and workgroup, the partial sums of dW2 and seven vector rows (db1, db2, dgamma, dbeta, dW1[:, 0..2]); one
    reduction launch per member finishes them (straight into the flat gradient views under the trainer).  No dz1 / dz2
    round trip, no weight-gradient launches behind the kernel.  Returns False when the library has no such kernel."""
    lib = L.load()
    params = ctx.params
    dev = params[0][0].device
    m = len(live)
    arr = (L.MlpBwd * m)()
    tiles = (C.c_int64 * m)()
    for i, k in enumerate(live):
        t, B, bstride, rows, W1c, W2c, z1, xhat, rstd = ctx.saved[k]
        tiles[i] = ((rows + 31) // 32) * B
    blocks = (C.c_int32 * m)()
    L.check(lib.nlam_mlp_group_blocks(tiles, m, blocks), "nlam_mlp_group_blocks")
    work = []
    for i, k in enumerate(live):
        t, B, bstride, rows, W1c, W2c, z1, xhat, rstd = ctx.saved[k]
        hid, kin = W1c.shape
        dout = W2c.shape[0]
        g = g_outs[k].reshape(B, rows, dout).contiguous()
        p = arr[i]
        _fill_src(p.src[0], t, bstride, kin, None)
        p.nsrc, p.batch, p.rows, p.ntiles = 1, B, rows, (rows + 31) // 32
        p.W1, p.W2, p.ln_w = _ptr(W1c), _ptr(W2c), _ptr(params[k][4])
        p.hid, p.dout, p.flags = hid, dout, ctx.mm_flags | L.F_LEAF_WGRAD
        p.g_out, p.out_bstride = _ptr(g), rows * dout
        p.z1, p.xhat, p.rstd = _ptr(z1), _ptr(xhat), _ptr(rstd)
        _set_bwd_pack(p, ctx.packs[k])
        b1c = params[k][1].contiguous()
        p.b1 = _ptr(b1c)
        nblk = int(blocks[i])
        vs = _vec_stride(hid, dout)
        dw2p = torch.empty((nblk, dout, hid), device=dev, dtype=torch.float32)
        vecp = torch.empty((nblk, 7, vs), device=dev, dtype=torch.float32)
        p.dz2, p.vec_partials, p.vec_partials_rows, p.vec_stride = _ptr(dw2p), _ptr(vecp), nblk, vs
        work.append((k, g, dw2p, vecp, nblk, vs, b1c))
    rows_all = sum(int(arr[i].rows) * int(arr[i].batch) for i in range(m))

    def meta():
        fl = sum(4.0 * arr[i].rows * arr[i].batch * arr[i].hid * arr[i].dout for i in range(m))
        # reads g_out, xhat, rstd and the <= 3 input columns (z1 is recomputed, dz1 / dz2 never leave the chip); writes one
        # (dout x hid) partial + seven vector rows per workgroup
        by = sum(4.0 * arr[i].rows * arr[i].batch * (2 * arr[i].dout + arr[i].src[0].width + 1) for i in range(m))
        by += sum(4.0 * w[4] * (arr[0].dout * arr[0].hid + 7 * w[5]) for w in work)
        name, mf = _mm_executed(ctx.mm_flags, arr[0].hid, arr[0].dout, [32])
        return {"flops": fl, "bytes": by, "mm": name, "mfmas_per_block": mf,
                "what": f"backward of {m} static-feature embedders in one grouped launch, weight gradients accumulated in the kernel"}

    if lib.nlam_mlp_bwd_family(arr) != 0:   # the fused-weight-gradient kernel is a narrow one
        return False

    # A dead end of backward (nothing upstream of a static-feature embedder needs a gradient): under a trainer that owns the
    # parameter gradients the launch and its reduction go to a weight-gradient side stream.  At the end of backward that changes
    # nothing; for an embedder whose output gradient is complete EARLY (early_backward_leaf: the m2g edge embedding right behind
    # the decoder's backward) it takes 64 % of this kernel's rows out of the tail of the step (round 6).
    all_direct = all(_all_direct(params[k], ctx.needs_input_grad[1 + 6 * k : 7 + 6 * k]) for (k, *_r) in work)
    if OVERLAP.active and all_direct:
        hold = [t_ for (k, g, dw2p, vecp, nblk, vs, b1c) in work for t_ in (g, dw2p, vecp, b1c, *[x_ for x_ in ctx.saved[k] if isinstance(x_, torch.Tensor)])]
        hold += [pk_.bwd for pk_ in ctx.packs if pk_ is not None and getattr(pk_, "bwd", None) is not None]
        OVERLAP.run(params[work[0][0]][0], hold, lambda: _grouped_backward_fused_launch(ctx, arr, m, work, rows_all, meta, grads), dead_end=True)
    else:
        _grouped_backward_fused_launch(ctx, arr, m, work, rows_all, meta, grads)
    return True


def _grouped_backward_fused_launch(ctx, arr, m, work, rows_all, meta, grads):
    lib = L.load()
    params = ctx.params
    rc = PROFILE.launch(("mlp_bwd_group_lw", rows_all, m, int(arr[0].hid), int(arr[0].dout)), lambda: lib.nlam_mlp_bwd_group(arr, m, _stream()), meta)
    if rc == -2:
        raise RuntimeError("nlam_mlp_bwd_group has no fused-weight-gradient kernel for a shape the forward planned it for")
    L.check(rc, "nlam_mlp_bwd_group (fused weight gradients)")

    batch = _ReduceBatch(params[0][0].device)   # ONE reduction launch for all members (<= 9 jobs each): they were four serial launches at the very end of the step
    done = []
    for (k, g, dw2p, vecp, nblk, vs, _b1c) in work:
        prm = params[k]
        hid, kin = prm[0].shape
        dout = prm[2].shape[0]
        needs = [ctx.needs_input_grad[1 + 6 * k + q] for q in range(6)]
        batch.reserve(9)
        out = None
        if needs[0]:   # dW1[:, c] = vector row 4 + c, scattered into column c of the (hid, kin) matrix
            for c in range(kin):
                out, direct = batch.add(vecp.data_ptr() + (4 + c) * vs * 4, nblk, 7 * vs, (hid, kin), prm[0], ncols=1, out=out, out_off=c)
        res = _mlp_reduce_jobs(batch, None, dw2p if needs[2] else None, vecp, nblk, vs, 7, (hid, kin, dout), prm, needs, prm[4] is not None)
        if out is not None and not direct:
            res[0] = out
        grads[6 * k : 6 * k + 6] = res
        done.append([q for q, nd in zip(prm, needs) if nd and q is not None and _direct_grad(q, q.shape)])
    batch.flush()
    if GRAD_LISTENER is not None:
        for d in done:
            GRAD_LISTENER.note_done(d)
    if OVERLAP.active and not OVERLAP.capturing and OVERLAP.deferred is None:
        OVERLAP.hold(torch.cuda.current_stream(), *batch.keep)


def _linear_launch(x2d, W, ldn, ldk, k, n, out=None, accumulate=False, mm_flags=None, W2=None, out2=None):
    """out (rows, n) (+)= x2d (rows, k) . A^T with A[h][c] = W[h * ldn + c * ldk] (nlam_linear); with W2 / out2 a second
    product over the same rows in the same launch."""
    lib = L.load()
    rows = x2d.shape[0]
    if out is None:
        out = torch.empty((rows, n), device=x2d.device, dtype=torch.float32)
    q = L.Linear()
    q.x, q.W, q.out, q.rows, q.ldn, q.ldk, q.k, q.n = _ptr(x2d), W, _ptr(out), rows, ldn, ldk, k, n
    q.accumulate, q.flags = 1 if accumulate else 0, mm_flags if mm_flags is not None else _mm_flags()
    if W2 is not None:
        q.W2, q.out2 = W2, _ptr(out2)
    key = ("linear", rows, k, n * (2 if W2 is not None else 1))
    L.check(PROFILE.launch(key, lambda: lib.nlam_linear(C.byref(q), _stream()),
                           lambda: {"flops": 2.0 * rows * k * key[3], "bytes": 4.0 * rows * (k + key[3]), "mm": _MM_NAMES[(q.flags >> 8) & 3],
                                    "mfmas_per_block": ((q.flags >> 8) & 3) * (((q.flags >> 8) & 3) + 1) // 2,
                                    "what": "node-level product of the factorised edge MLP"}), "nlam_linear")
    return out


class NodeLinearFunction(torch.autograd.Function):
    """``x @ W1[:, col0 : col0 + k].T`` per NODE: one of the two node-level products of the factorised edge MLP
    (``edge_mlp(cat(e, x_j, x_i))`` of gnn_layers.py:168-172 with the first Linear split by column blocks).

    forward(x (..., N, k), W1 (hid, kin), col0) -> (..., N, hid).  A batch that is a stride-0 expansion is computed
    once.  Backward: dx = g @ W1[:, col0 : col0 + k] (nlam_linear, transposed strides), dW1[:, col0 : col0 + k] = g^T x
    (nlam_wgrad + nlam_reduce_jobs with a strided destination, on a weight-gradient side stream under the trainer)."""

    @staticmethod
    def forward(ctx, x, W1, col0: int, mail: bool = False):
        if x.dtype != torch.float32 and x.is_floating_point():
            x = x.float()   # storage is fp32 throughout (autocast regions hand in low-precision activations)
        _require_gpu(x, W1)
        xb, B, bstride, lead = as_batched(x)
        N, k = xb.shape[-2], xb.shape[-1]
        hid, kin = W1.shape
        shared = bstride == 0 and B > 1
        x2d = xb.reshape(-1, k)
        W1c = W1.contiguous()
        mm = _mm_flags()
        out = _linear_launch(x2d, W1c.data_ptr() + 4 * col0, kin, 1, k, hid, mm_flags=mm)
        ctx.save_for_backward(x2d, W1c)
        ctx.meta = (col0, tuple(x.shape), B, N, shared, mm)
        ctx.param_ref = W1
        ctx.mail = MAIL_TOKEN if (mail and MAIL_TOKEN is not None and not shared and ctx.needs_input_grad[0]) else None
        if ctx.mail is not None:
            _MAIL_CONSUMERS.add(ctx.mail)
        if GRAD_LISTENER is not None and W1.requires_grad:
            GRAD_LISTENER.note_use([W1])   # W1 collects gradient from the edge kernel AND from both node-level products
        ctx.set_materialize_grads(False)
        out = out.reshape(N, hid).expand(*lead, N, hid) if shared else out.reshape(*lead, N, hid)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            if ctx.mail is not None:
                _MAILBOX.pop(ctx.mail, None)   # nothing to add: the posted buffer already is the whole gradient autograd holds
            return None, None, None, None
        lib = L.load()
        x2d, W1 = ctx.saved_tensors
        col0, xshape, B, N, shared, mm = ctx.meta
        hid, kin = W1.shape
        k = x2d.shape[1]
        dev = g.device
        g2d = g.reshape(B, N, hid).sum(0) if shared else g.reshape(-1, hid)
        g2d = g2d.contiguous()
        rows = g2d.shape[0]
        dx = None
        if ctx.needs_input_grad[0]:
            posted = _MAILBOX.pop(ctx.mail, None) if ctx.mail is not None else None
            if posted is not None and posted.numel() == rows * k and posted.is_contiguous():
                # the node MLP of this layer has already written its gradient of x: add this product's on top, report nothing
                MAIL_STATS["consumed"] += 1
                _linear_launch(g2d, W1.data_ptr() + 4 * col0, 1, kin, hid, k, out=posted.view(rows, k), accumulate=True, mm_flags=mm)
            else:
                dx = _linear_launch(g2d, W1.data_ptr() + 4 * col0, 1, kin, hid, k, mm_flags=mm)
                dx = dx.reshape(N, k).expand(xshape) if shared else dx.reshape(xshape)
        dW = None
        if ctx.needs_input_grad[1]:
            dW = _node_linear_wgrad(ctx.param_ref, [(g2d, col0)], x2d, mm)
        return dx, dW, None, None


def _node_linear_wgrad(prm, g_cols, x2d, mm):
    """dW1[:, col0 : col0 + k] (+)= g^T x for each (g (rows, hid), col0): nlam_wgrad + one strided reduction launch; on a
    weight-gradient side stream and straight into the flat gradient view under the trainer (returns None then)."""
    lib = L.load()
    hid, kin = prm.shape
    rows, k = x2d.shape
    dev = x2d.device
    direct = _direct_grad(prm, (hid, kin))
    on_side = OVERLAP.active and direct
    out = prm.grad if direct else torch.zeros((hid, kin), device=dev, dtype=torch.float32)

    def launch():
        batch = _ReduceBatch(dev)
        parts = []
        for g2d, col0 in g_cols:
            q, partials = _wgrad_request(g2d, hid, k, 1, rows, [(x2d, 0, k, None)], mm | _wgrad_solo(), dev)
            nparts = partials.shape[0]
            parts.append(partials)
            key = ("wgrad", rows, hid, k)
            L.check(PROFILE.launch(key, lambda: lib.nlam_wgrad(C.byref(q), _stream()),
                                   lambda: {"flops": 2.0 * rows * hid * k, "bytes": 4.0 * (rows * (hid + k) + nparts * hid * k), "bytes_min": 4.0 * (rows * (hid + k) + hid * k),
                                            "mm": "f32" if max(hid, k) <= 64 else _MM_NAMES[(mm >> 8) & 3],
                                            "mfmas_per_block": 0 if max(hid, k) <= 64 else ((mm >> 8) & 3) * (((mm >> 8) & 3) + 1) // 2,
                                            "what": "node-level weight gradient of the factorised edge MLP"}), "nlam_wgrad")
            batch.add(_ptr(partials), nparts, hid * k, (hid, kin), prm, ncols=k, out=out, out_off=col0)
        batch.flush()
        if on_side:
            OVERLAP.hold(torch.cuda.current_stream(), *parts)
        if GRAD_LISTENER is not None and direct:
            GRAD_LISTENER.note_done([prm])

    if on_side:
        OVERLAP.run(prm, (x2d, *[g for g, _ in g_cols]), launch)
    else:
        launch()
    return None if direct else out


class NodeLinearPairFunction(torch.autograd.Function):
    """Both node-level products of a layer whose senders are its receivers (mesh <-> mesh), widths above 64:
    ``(x @ W1[:, cj : cj + k].T, x @ W1[:, ci : ci + k].T)`` in ONE launch (nlam_linear with W2 / out2); backward: one
    data-gradient launch pair accumulating into one dx, both column blocks of dW1 from one reduction launch."""

    @staticmethod
    def forward(ctx, x, W1, cj: int, ci: int, mail: bool = False):
        if x.dtype != torch.float32 and x.is_floating_point():
            x = x.float()
        _require_gpu(x, W1)
        xb, B, bstride, lead = as_batched(x)
        N, k = xb.shape[-2], xb.shape[-1]
        hid, kin = W1.shape
        shared = bstride == 0 and B > 1
        x2d = xb.reshape(-1, k)
        W1c = W1.contiguous()
        mm = _mm_flags()
        pj = torch.empty((x2d.shape[0], hid), device=x.device, dtype=torch.float32)
        pi = torch.empty_like(pj)
        _linear_launch(x2d, W1c.data_ptr() + 4 * cj, kin, 1, k, hid, out=pj, mm_flags=mm, W2=W1c.data_ptr() + 4 * ci, out2=pi)
        ctx.save_for_backward(x2d, W1c)
        ctx.meta = (cj, ci, tuple(x.shape), B, N, shared, mm)
        ctx.param_ref = W1
        ctx.set_materialize_grads(False)
        ctx.mail = MAIL_TOKEN if (mail and MAIL_TOKEN is not None and not shared and ctx.needs_input_grad[0]) else None
        if ctx.mail is not None:
            _MAIL_CONSUMERS.add(ctx.mail)
        if GRAD_LISTENER is not None and W1.requires_grad:
            GRAD_LISTENER.note_use([W1])
        shape = lambda t: t.reshape(N, hid).expand(*lead, N, hid) if shared else t.reshape(*lead, N, hid)  # noqa: E731
        return shape(pj), shape(pi)

    @staticmethod
    def backward(ctx, gj, gi):
        if gj is None and gi is None:
            if ctx.mail is not None:
                _MAILBOX.pop(ctx.mail, None)
            return None, None, None, None, None
        x2d, W1 = ctx.saved_tensors
        cj, ci, xshape, B, N, shared, mm = ctx.meta
        hid, kin = W1.shape
        k = x2d.shape[1]
        prep = lambda g: None if g is None else (g.reshape(B, N, hid).sum(0) if shared else g.reshape(-1, hid)).contiguous()  # noqa: E731
        gj2, gi2 = prep(gj), prep(gi)
        dx = None
        if ctx.needs_input_grad[0]:
            posted = _MAILBOX.pop(ctx.mail, None) if ctx.mail is not None else None
            if posted is not None and posted.numel() == x2d.numel() and posted.is_contiguous():
                dx = posted.view(x2d.shape)   # the node MLP's gradient of x, already written: both products are added on top
                MAIL_STATS["consumed"] += 1
            else:
                posted = None
            for g2d, c0 in ((gj2, cj), (gi2, ci)):
                if g2d is not None:
                    dx = _linear_launch(g2d, W1.data_ptr() + 4 * c0, 1, kin, hid, k, out=dx, accumulate=dx is not None, mm_flags=mm)
            if posted is not None:
                dx = None   # nothing to report: autograd already holds the buffer
            else:
                dx = dx.reshape(N, k).expand(xshape) if shared else dx.reshape(xshape)
        dW = None
        if ctx.needs_input_grad[1]:
            dW = _node_linear_wgrad(ctx.param_ref, [(g, c) for g, c in ((gj2, cj), (gi2, ci)) if g is not None], x2d, mm)
        return dx, dW, None, None, None


def _cont(t):
    return None if t is None else t.contiguous()


_LOSS_NPARTS = 512   # workgroups (= partial sums) of a loss pass


def _scalar_from_partials(device, launch, what):
    """The scalar a loss pass leaves behind: ``launch(partials address, nparts)`` writes one partial sum per workgroup,
    nlam_reduce_partials adds them in a fixed order."""
    lib = L.load()
    partials = torch.empty((_LOSS_NPARTS,), device=device, dtype=torch.float32)
    L.check(launch(_ptr(partials), _LOSS_NPARTS), what)
    out = torch.empty((), device=device, dtype=torch.float32)
    L.check(lib.nlam_reduce_partials(_ptr(partials), _LOSS_NPARTS, 1, 1, _ptr(out), 0, _stream()), "nlam_reduce_partials")
    return out


class WmseLossFunction(torch.autograd.Function):
    """``mean_t mean_b wmse(pred, target, per_var_std, interior mask)`` as one pass (nlam_wmse_fwd / _bwd).

    forward(pred (B, T, N, V), target, inv_var (V), row_weight (N) = interior / #interior) -> scalar
    """

    @staticmethod
    def forward(ctx, pred, target, inv_var, row_weight):
        lib = L.load()
        _require_gpu(pred, target, inv_var, row_weight)
        B, T, N, V = pred.shape
        predc, targc = pred.contiguous(), target.contiguous()
        scale = 1.0 / (B * T)
        out = _scalar_from_partials(pred.device, lambda partials, nparts: lib.nlam_wmse_fwd(
            _ptr(predc), _ptr(targc), _ptr(inv_var), _ptr(row_weight), B * T * N, N, V, scale, partials, nparts, _stream()),
            "nlam_wmse_fwd")
        ctx.save_for_backward(predc, targc, inv_var, row_weight)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        pred, target, inv_var, row_weight = ctx.saved_tensors
        B, T, N, V = pred.shape
        dpred = torch.empty_like(pred)
        gc = g.contiguous().to(torch.float32)
        L.check(lib.nlam_wmse_bwd(_ptr(pred), _ptr(target), _ptr(inv_var), _ptr(row_weight), _ptr(gc), B * T * N, N, V,
                                  ctx.scale, _ptr(dpred), _stream()), "nlam_wmse_bwd")
        return dpred, None, None, None


def _affine_mix(x, a, y, c, z, s, m, like):
    """out = a[node] * x + c[node] * (y + z * s[var] + m[var]) on (..., N, F) fp32 tensors; any term may be None."""
    lib = L.load()
    N, F = like.shape[-2], like.shape[-1]
    out = torch.empty(like.shape, device=like.device, dtype=torch.float32)
    rc = lib.nlam_affine_mix(_ptr(x), _ptr(a), _ptr(y), _ptr(c), _ptr(z), _ptr(s), _ptr(m), _ptr(out),
                             out.numel() // F, N, F, _stream())
    L.check(rc, "nlam_affine_mix")
    return out


class AffineMixFunction(torch.autograd.Function):
    """One pass for the elementwise tail of an autoregressive step (include/nlam_hip.h, nlam_affine_mix):

        out = a * x + c * (y + z * s + m)        a, c: per node (N,) or None; s, m: per variable (F,) or None

    ``prev_state + (delta * diff_std + diff_mean)`` is (y = prev, z = delta, s, m); the boundary overwrite
    ``boundary_mask * truth + interior_mask * pred`` is (a, x = truth, c, y = pred).  Gradients flow to y and z (x is
    data, a / c / s / m are buffers); each is the same kernel with the operands permuted."""

    @staticmethod
    def forward(ctx, x, a, y, c, z, s, m):
        like = y if y is not None else z
        tens = [t for t in (x, a, y, c, z, s, m) if t is not None]
        _require_gpu(*tens)
        x, a, y, c, z, s, m = map(_cont, (x, a, y, c, z, s, m))
        ctx.save_for_backward(c, s)
        return _affine_mix(x, a, y, c, z, s, m, like)

    @staticmethod
    def backward(ctx, g):
        c, s = ctx.saved_tensors
        g = g.contiguous()
        gy = gz = None
        if ctx.needs_input_grad[2]:
            gy = _affine_mix(None, None, g, c, None, None, None, g) if c is not None else g
        if ctx.needs_input_grad[4]:
            gz = _affine_mix(None, None, None, c, g, s, None, g)
        return None, None, gy, None, gz, None, None


class StepTailFunction(torch.autograd.Function):
    """The elementwise tail of one AR step in one pass each way:

        new = prev + delta * diff_std + diff_mean ; pred = bmask * truth + (1 - bmask) * new ;
        loss_t = scale * sum_n,f row_weight[n] * entry(pred - target; consts[f])

    i.e. ``step_predictors/graph/base.py:331-343`` + ``forecasters/autoregressive.py:128-131`` + this step's term of the
    loss (``metrics.py`` / ``module.py:463-510``; three elementwise launches + the loss pass in the reference's formulation,
    and as many again in backward).  ``kind=None`` is the default wmse with ``consts = inv_var = 1 / std^2`` handed in
    (nlam_step_tail_fwd / _bwd); a ``_lib.LOSS_*`` kind takes ``consts = var_std``, the per-variable std, None for mse /
    mae (nlam_step_tail_loss_fwd / _bwd).  forward(delta, prev, truth, target, dstd, dmean, bmask (N,), consts (F,),
    row_weight (N,), scale, kind) -> (pred (B, N, F), loss_t scalar)."""

    @staticmethod
    def _entry(lib, name, kind):
        """(entry point of this kind, its name): the _loss_ pair takes the kind as its first argument"""
        if kind is None:
            return getattr(lib, f"nlam_step_tail_{name}"), f"nlam_step_tail_{name}"
        f = getattr(lib, f"nlam_step_tail_loss_{name}")
        return (lambda *args: f(kind, *args)), f"nlam_step_tail_loss_{name}"

    @staticmethod
    def forward(ctx, delta, prev, truth, target, dstd, dmean, bmask, consts, row_weight, scale: float, kind=None):
        _require_gpu(delta, prev, truth, target, dstd, dmean, bmask, consts, row_weight)
        B, N, F = delta.shape
        delta, prev, truth, target = map(_cont, (delta, prev, truth, target))
        pred = torch.empty((B, N, F), device=delta.device, dtype=torch.float32)
        fwd, what = StepTailFunction._entry(L.load(), "fwd", kind)
        loss = _scalar_from_partials(delta.device, lambda partials, nparts: fwd(
            _ptr(delta), _ptr(prev), _ptr(truth), _ptr(target), _ptr(dstd), _ptr(dmean), _ptr(bmask), _ptr(consts), _ptr(row_weight),
            scale, _ptr(pred), partials, nparts, B * N, N, F, _stream()), what)
        ctx.save_for_backward(pred, target, dstd, bmask, consts, row_weight)
        ctx.scale, ctx.kind = scale, kind
        ctx.set_materialize_grads(False)
        return pred, loss

    @staticmethod
    def backward(ctx, g_pred, g_loss):
        pred, target, dstd, bmask, consts, row_weight = ctx.saved_tensors
        B, N, F = pred.shape
        if g_pred is None and g_loss is None:
            return (None,) * 11
        dev = pred.device
        gl = g_loss.contiguous().to(torch.float32) if g_loss is not None else torch.zeros((), device=dev, dtype=torch.float32)
        gp = g_pred.contiguous() if g_pred is not None else None
        d_delta = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        d_prev = torch.empty_like(pred) if ctx.needs_input_grad[1] else None
        if d_delta is None and d_prev is None:
            return (None,) * 11
        bwd, what = StepTailFunction._entry(L.load(), "bwd", ctx.kind)
        L.check(bwd(_ptr(gp), _ptr(gl), _ptr(pred), _ptr(target), _ptr(dstd), _ptr(bmask), _ptr(consts), _ptr(row_weight), ctx.scale,
                    _ptr(d_delta), _ptr(d_prev), B * N, N, F, _stream()), what)
        return d_delta, d_prev, None, None, None, None, None, None, None, None, None


class ClampTables:
    """The per-variable output clamps of a step predictor as nlam_step_tail_t takes them: ``mode`` (F,) NLAM_CLAMP_* per
    variable in host memory, ``lo`` / ``hi`` (F,) fp32 standardised limits on the device (0 where a variable has no such limit)."""

    __slots__ = ("mode", "lo", "hi", "modes")

    def __init__(self, modes, lo, hi):
        self.modes = tuple(int(m) for m in modes)
        self.mode = (C.c_int32 * len(self.modes))(*self.modes)
        self.lo, self.hi = lo, hi

    def __reduce__(self):   # the ctypes array is rebuilt from the modes: a module that holds its tables copies and pickles
        return ClampTables, (self.modes, self.lo, self.hi)


class StepTailExtFunction(torch.autograd.Function):
    """StepTailFunction for a predictor with output clamping and / or a predicted std, still one pass each way
    (nlam_step_tail_ext_fwd / _bwd; the formulas are in include/nlam_hip.h):

    forward(delta (B, N, F | 2 F), prev, truth, target | None, dstd, dmean, bmask (N,), consts (F,) | None, row_weight (N,) | None,
    scale, kind | None, clamp: ClampTables | None) -> (pred (B, N, F), pred_std (B, N, F) | None, loss_t scalar | None).
    ``delta`` of width 2 F carries the raw std in its second half.  ``target=None``: no loss term (inference, evaluation, a loss
    computed outside: the gradients then arrive through pred and pred_std).  ``consts`` is the per-variable std of ``kind``, None
    with a predicted std and for mse / mae."""

    @staticmethod
    def _args(delta, prev, target, dstd, dmean, bmask, consts, row_weight, scale, kind, clamp, pred, pred_std):
        B, N, F = prev.shape
        p = L.StepTail()
        p.delta, p.prev, p.target, p.dstd, p.dmean = _ptr(delta), _ptr(prev), _ptr(target), _ptr(dstd), _ptr(dmean)
        p.bmask, p.row_weight, p.consts = _ptr(bmask), _ptr(row_weight), _ptr(consts)
        if clamp is not None:
            p.clamp_mode_host, p.clamp_lo, p.clamp_hi = C.addressof(clamp.mode), _ptr(clamp.lo), _ptr(clamp.hi)
        p.pred, p.pred_std = _ptr(pred), _ptr(pred_std)
        p.rows, p.nodes, p.nvars, p.delta_ld = B * N, N, F, delta.shape[-1]
        p.kind, p.scale = (kind if kind is not None else L.LOSS_MSE), scale
        return p

    @staticmethod
    def forward(ctx, delta, prev, truth, target, dstd, dmean, bmask, consts, row_weight, scale: float, kind=None, clamp=None):
        lib = L.load()
        tables = () if clamp is None else (clamp.lo, clamp.hi)
        _require_gpu(*(t for t in (delta, prev, truth, target, dstd, dmean, bmask, consts, row_weight, *tables) if t is not None))
        B, N, F = prev.shape
        if delta.shape[-1] not in (F, 2 * F):
            raise ValueError(f"StepTailExtFunction: delta of width {delta.shape[-1]} for {F} state variables")
        if clamp is not None and len(clamp.modes) != F:
            raise ValueError(f"StepTailExtFunction: {len(clamp.modes)} clamp modes for {F} state variables")
        delta, prev, truth, target = map(_cont, (delta, prev, truth, target))
        dev = prev.device
        pred = torch.empty((B, N, F), device=dev, dtype=torch.float32)
        pred_std = torch.empty((B, N, F), device=dev, dtype=torch.float32) if delta.shape[-1] == 2 * F else None
        p = StepTailExtFunction._args(delta, prev, target, dstd, dmean, bmask, consts, row_weight, scale, kind, clamp, pred, pred_std)
        p.truth = _ptr(truth)
        loss = None
        if target is None:
            L.check(lib.nlam_step_tail_ext_fwd(C.byref(p), _stream()), "nlam_step_tail_ext_fwd")
        else:
            def launch(partials, nparts):
                p.partials, p.nparts = partials, nparts
                return lib.nlam_step_tail_ext_fwd(C.byref(p), _stream())

            loss = _scalar_from_partials(dev, launch, "nlam_step_tail_ext_fwd")
        ctx.save_for_backward(delta, prev, pred, pred_std, target, dstd, dmean, bmask, consts, row_weight, *tables)
        ctx.scale, ctx.kind, ctx.clamp = scale, kind, clamp
        ctx.set_materialize_grads(False)
        return pred, pred_std, loss

    @staticmethod
    def backward(ctx, g_pred, g_std, g_loss):
        delta, prev, pred, pred_std, target, dstd, dmean, bmask, consts, row_weight = ctx.saved_tensors[:10]
        none = (None,) * 12
        if (g_pred is None and g_std is None and g_loss is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return none
        dev = prev.device
        gl = None
        if target is not None:
            gl = g_loss.contiguous().to(torch.float32) if g_loss is not None else torch.zeros((), device=dev, dtype=torch.float32)
        gp = g_pred.contiguous() if g_pred is not None else None
        gs = g_std.contiguous() if g_std is not None else None
        d_delta = torch.empty_like(delta)
        d_prev = torch.empty_like(prev) if ctx.needs_input_grad[1] else None
        p = StepTailExtFunction._args(delta, prev, target, dstd, dmean, bmask, consts, row_weight, ctx.scale, ctx.kind, ctx.clamp,
                                      pred, pred_std)
        p.g_pred, p.g_std, p.gloss, p.d_delta, p.d_prev = _ptr(gp), _ptr(gs), _ptr(gl), _ptr(d_delta), _ptr(d_prev)
        L.check(L.load().nlam_step_tail_ext_bwd(C.byref(p), _stream()), "nlam_step_tail_ext_bwd")
        return (d_delta if ctx.needs_input_grad[0] else None, d_prev) + none[2:]


class LossFunction(torch.autograd.Function):
    """``mean_t mean_b metrics.<kind>(pred, target, std, interior mask)`` as one pass each way (nlam_loss_fwd / _bwd) for every
    ``--loss`` kind (``_lib.LOSS_*``).  The std is per entry (``pred_std``, an output_std model's prediction) or, with
    ``pred_std=None``, per variable (``var_std`` (V,)); mse / mae read neither.

    forward(pred (B, T, N, V), target, pred_std (B, T, N, V) | None, var_std (V) | None, row_weight (N) = interior / #interior,
    kind) -> scalar.  Gradients: pred, and pred_std when it requires one."""

    @staticmethod
    def _args(pred, target, pred_std, var_std, row_weight, kind, scale):
        B, T, N, V = pred.shape
        p = L.Loss()
        p.pred, p.target, p.std = _ptr(pred), _ptr(target), _ptr(pred_std)
        p.var_std, p.row_weight = _ptr(var_std), _ptr(row_weight)
        p.rows, p.nodes, p.nvars, p.kind, p.scale = B * T * N, N, V, kind, scale
        return p

    @staticmethod
    def forward(ctx, pred, target, pred_std, var_std, row_weight, kind: int):
        lib = L.load()
        _require_gpu(*(t for t in (pred, target, pred_std, var_std, row_weight) if t is not None))
        B, T = pred.shape[0], pred.shape[1]
        pred, target, pred_std = map(_cont, (pred, target, pred_std))
        scale = 1.0 / (B * T)
        p = LossFunction._args(pred, target, pred_std, var_std, row_weight, kind, scale)

        def launch(partials, nparts):
            p.partials, p.nparts = partials, nparts
            return lib.nlam_loss_fwd(C.byref(p), _stream())

        out = _scalar_from_partials(pred.device, launch, "nlam_loss_fwd")
        ctx.save_for_backward(pred, target, pred_std, var_std, row_weight)
        ctx.kind, ctx.scale = kind, scale
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        pred, target, pred_std, var_std, row_weight = ctx.saved_tensors
        p = LossFunction._args(pred, target, pred_std, var_std, row_weight, ctx.kind, ctx.scale)
        gc = g.contiguous().to(torch.float32)
        dpred = torch.empty_like(pred)
        dstd = torch.empty_like(pred_std) if pred_std is not None and ctx.needs_input_grad[2] else None
        p.gscalar, p.dpred, p.dstd = _ptr(gc), _ptr(dpred), _ptr(dstd)
        L.check(lib.nlam_loss_bwd(C.byref(p), _stream()), "nlam_loss_bwd")
        return dpred, None, dstd, None, None, None


class LatentKLFunction(torch.autograd.Function):
    """The posterior draw and the KL term of one AR step of the Graph-EFM objective (nlam_latent_kl_fwd / _bwd; the formulas are
    in include/nlam_hip.h):

    forward(pq (B, R, 2 D), pp (B, R, D | 2 D), kl_weight (device float), seed (device word: the 64 bits of the key), draw (device int64), t,
    noise_in (B, R, D) | None) -> (z (B, R, D), kl_term scalar = kl_weight * sum_b KL_b, kl_per_item (B,)).
    ``z = mu_q + s_q eps``; eps is drawn on the device under (seed, draw, t) unless ``noise_in`` is given, and saved for the
    backward with pq and pp.  Gradients: pq, and pp when it requires one (a constant prior gets none); ``kl_per_item`` is not
    differentiable.  No host synchronisation, no allocation outside torch's allocator: the call can be captured.  ``kl_weight`` is
    saved for the backward, which multiplies it in again: writing it in place between an eager forward and its backward makes
    autograd refuse the backward, and a replayed backward reads the word as it is then."""

    @staticmethod
    def _args(pq, pp, kl_weight, eps, t):
        B, R, D2 = pq.shape
        D = D2 // 2
        if D2 != 2 * D or pp.dim() != 3 or pp.shape[:2] != (B, R) or pp.shape[2] not in (D, 2 * D):
            raise ValueError(f"LatentKLFunction: posterior parameters {tuple(pq.shape)} against prior parameters {tuple(pp.shape)}")
        p = L.LatentKl()
        p.pq, p.pp, p.kl_weight, p.eps = _ptr(pq), _ptr(pp), _ptr(kl_weight), _ptr(eps)
        p.batch, p.rows, p.latent_dim, p.diagonal, p.t = B, R, D, int(pp.shape[2] == 2 * D), int(t)
        return p

    @staticmethod
    def forward(ctx, pq, pp, kl_weight, seed, draw, t: int, noise_in=None):
        lib = L.load()
        _require_gpu(pq, pp, kl_weight, noise_in)
        if noise_in is None and not (seed.is_cuda and draw.is_cuda and seed.dtype in (torch.uint64, torch.int64) and draw.dtype == torch.int64):
            raise RuntimeError("LatentKLFunction: seed (the 64 bits of the key, uint64 or int64) and draw (int64) are words in device memory")
        pq, pp, noise_in = map(_cont, (pq, pp, noise_in))
        B, R, D = pq.shape[0], pq.shape[1], pq.shape[2] // 2
        dev = pq.device
        eps = torch.empty((B, R, D), device=dev, dtype=torch.float32)
        p = LatentKLFunction._args(pq, pp, kl_weight, eps, t)
        if noise_in is not None and noise_in.shape != eps.shape:
            raise ValueError(f"LatentKLFunction: noise of shape {tuple(noise_in.shape)} for a latent of shape {tuple(eps.shape)}")
        z = torch.empty_like(eps)
        kl = torch.empty((B,), device=dev, dtype=torch.float32)
        kl_term = torch.empty((), device=dev, dtype=torch.float32)
        nws = lib.nlam_latent_kl_workspace_floats(B, R, D)
        if nws < 0:
            L.check(int(nws), "nlam_latent_kl_workspace_floats")
        ws = torch.empty((nws,), device=dev, dtype=torch.float32)
        p.noise_in, p.latent, p.kl, p.kl_term, p.workspace, p.workspace_floats = _ptr(noise_in), _ptr(z), _ptr(kl), _ptr(kl_term), _ptr(ws), nws
        if noise_in is None:
            p.seed, p.draw = _ptr(seed), _ptr(draw)
        L.check(lib.nlam_latent_kl_fwd(C.byref(p), _stream()), "nlam_latent_kl_fwd")
        ctx.save_for_backward(pq, pp, eps, kl_weight)
        ctx.t = int(t)
        ctx.mark_non_differentiable(kl)
        ctx.set_materialize_grads(False)
        return z, kl_term, kl

    @staticmethod
    def backward(ctx, g_z, g_term, _g_kl):
        pq, pp, eps, kl_weight = ctx.saved_tensors
        none = (None,) * 7
        if (g_z is None and g_term is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return none
        gt = g_term.contiguous().to(torch.float32) if g_term is not None else torch.zeros((), device=pq.device, dtype=torch.float32)
        gz = g_z.contiguous() if g_z is not None else None
        g_pq = torch.empty_like(pq)
        g_pp = torch.empty_like(pp) if ctx.needs_input_grad[1] else None
        p = LatentKLFunction._args(pq, pp, kl_weight, eps, ctx.t)
        p.g_latent, p.g_kl_term, p.g_pq, p.g_pp = _ptr(gz), _ptr(gt), _ptr(g_pq), _ptr(g_pp)
        L.check(L.load().nlam_latent_kl_bwd(C.byref(p), _stream()), "nlam_latent_kl_bwd")
        return (g_pq if ctx.needs_input_grad[0] else None, g_pp) + none[2:]


class LatentDrawFunction(torch.autograd.Function):
    """The prior draw of one AR step of the member rollout of the Graph-EFM CRPS term, with its gradient (nlam_latent_draw_fwd /
    _bwd; the formulas are in include/nlam_hip.h):

    forward(params (B, R, D | 2 D), latent_dim D, seed (device word: the 64 bits of the key), draw (device int64), t,
    noise_in (B, R, D) | None) -> z (B, R, D) = mean + std eps.
    eps is drawn on the device under (seed, draw, t) unless ``noise_in`` is given, and saved for the backward with ``params``.
    Gradient: ``params`` when it requires one (a constant prior gets none, and nothing is launched).  No host synchronisation, no
    allocation outside torch's allocator: the call can be captured."""

    @staticmethod
    def _args(params, D, eps, t):
        B, R, P = params.shape
        if P not in (D, 2 * D) or D < 1:
            raise ValueError(f"LatentDrawFunction: prior parameters {tuple(params.shape)} for a latent of width {D}")
        p = L.LatentDraw()
        p.params, p.eps = _ptr(params), _ptr(eps)
        p.batch, p.rows, p.latent_dim, p.diagonal, p.t = B, R, D, int(P == 2 * D), int(t)
        return p

    @staticmethod
    def forward(ctx, params, latent_dim: int, seed, draw, t: int, noise_in=None):
        _require_gpu(params, noise_in)
        if noise_in is None and not (seed.is_cuda and draw.is_cuda and seed.dtype in (torch.uint64, torch.int64) and draw.dtype == torch.int64):
            raise RuntimeError("LatentDrawFunction: seed (the 64 bits of the key, uint64 or int64) and draw (int64) are words in device memory")
        params, noise_in = map(_cont, (params, noise_in))
        B, R, D = params.shape[0], params.shape[1], int(latent_dim)
        eps = torch.empty((B, R, D), device=params.device, dtype=torch.float32)
        p = LatentDrawFunction._args(params, D, eps, t)
        if noise_in is not None and noise_in.shape != eps.shape:
            raise ValueError(f"LatentDrawFunction: noise of shape {tuple(noise_in.shape)} for a latent of shape {tuple(eps.shape)}")
        z = torch.empty_like(eps)
        p.noise_in, p.latent = _ptr(noise_in), _ptr(z)
        if noise_in is None:
            p.seed, p.draw = _ptr(seed), _ptr(draw)
        L.check(L.load().nlam_latent_draw_fwd(C.byref(p), _stream()), "nlam_latent_draw_fwd")
        ctx.save_for_backward(params, eps)
        ctx.t, ctx.latent_dim = int(t), D
        ctx.set_materialize_grads(False)
        return z

    @staticmethod
    def backward(ctx, g_z):
        params, eps = ctx.saved_tensors
        if g_z is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        g_z = g_z.contiguous()
        g_params = torch.empty_like(params)
        p = LatentDrawFunction._args(params, ctx.latent_dim, eps, ctx.t)
        p.g_latent, p.g_params = _ptr(g_z), _ptr(g_params)
        L.check(L.load().nlam_latent_draw_bwd(C.byref(p), _stream()), "nlam_latent_draw_bwd")
        return (g_params,) + (None,) * 5


class CrpsEnsFunction(torch.autograd.Function):
    """The unbiased ensemble CRPS of one AR step of the member rollout (nlam_crps_ens_fwd / _bwd; the formulas are in
    include/nlam_hip.h):

    forward(pred (B M, N, F), target (B, N, F), row_weight (N,), var_weight (F,) | None, weight (device float), members M) ->
    (term scalar = weight * sum_b crps_b, crps_per_item (B,)).  Item ``b * M + m`` of ``pred`` is member m of batch item b.
    Gradient: ``pred``, recomputed from ``pred`` and ``target`` (nothing else is saved); ``crps_per_item`` is not differentiable.
    ``weight`` is saved for the backward, which multiplies it in again, as ``LatentKLFunction`` treats ``kl_weight``.  No host
    synchronisation, no allocation outside torch's allocator: the call can be captured."""

    @staticmethod
    def _args(pred, target, row_weight, var_weight, weight, members):
        BM, N, F = pred.shape
        B = BM // members
        if members < 2 or B * members != BM or tuple(target.shape) != (B, N, F) or row_weight.numel() != N or (
                var_weight is not None and var_weight.numel() != F):
            raise ValueError(f"CrpsEnsFunction: {members} members, states {tuple(pred.shape)}, target {tuple(target.shape)}")
        p = L.CrpsEns()
        p.pred, p.target, p.row_weight, p.var_weight, p.weight = _ptr(pred), _ptr(target), _ptr(row_weight), _ptr(var_weight), _ptr(weight)
        p.batch, p.members, p.nodes, p.nvars = B, int(members), N, F
        return p

    @staticmethod
    def forward(ctx, pred, target, row_weight, var_weight, weight, members: int):
        lib = L.load()
        _require_gpu(pred, target, row_weight, var_weight, weight)
        pred, target, row_weight, var_weight = map(_cont, (pred, target, row_weight, var_weight))
        p = CrpsEnsFunction._args(pred, target, row_weight, var_weight, weight, members)
        B, dev = p.batch, pred.device
        crps = torch.empty((B,), device=dev, dtype=torch.float32)
        term = torch.empty((), device=dev, dtype=torch.float32)
        nws = lib.nlam_crps_ens_workspace_floats(B, int(members), p.nodes, p.nvars)
        if nws < 0:
            L.check(int(nws), "nlam_crps_ens_workspace_floats")
        ws = torch.empty((nws,), device=dev, dtype=torch.float32)
        p.crps, p.term, p.workspace, p.workspace_floats = _ptr(crps), _ptr(term), _ptr(ws), nws
        L.check(lib.nlam_crps_ens_fwd(C.byref(p), _stream()), "nlam_crps_ens_fwd")
        ctx.save_for_backward(pred, target, row_weight, var_weight, weight)
        ctx.members = int(members)
        ctx.mark_non_differentiable(crps)
        ctx.set_materialize_grads(False)
        return term, crps

    @staticmethod
    def backward(ctx, g_term, _g_crps):
        pred, target, row_weight, var_weight, weight = ctx.saved_tensors
        if g_term is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        gt = g_term.contiguous().to(torch.float32)
        g_pred = torch.empty_like(pred)
        p = CrpsEnsFunction._args(pred, target, row_weight, var_weight, weight, ctx.members)
        p.g_term, p.g_pred = _ptr(gt), _ptr(g_pred)
        L.check(L.load().nlam_crps_ens_bwd(C.byref(p), _stream()), "nlam_crps_ens_bwd")
        return (g_pred,) + (None,) * 5


def crps_ens_torch(pred, target, row_weight, var_weight, weight, members: int):
    """``CrpsEnsFunction`` composed from torch ops on the same member states (models.FUSED_CRPS off: the comparison route of the
    tests and of tools/efm_train_bench.py).  The (B, M, M, N, F) temporary of the pair term is what the kernel avoids."""
    BM, N, F = pred.shape
    B, M = BM // members, int(members)
    x = pred.reshape(B, M, N, F)
    wc = row_weight.reshape(N, 1) * (var_weight.reshape(1, F) if var_weight is not None else 1.0)
    skill = (x - target.unsqueeze(1)).abs().sum(1) / M
    pair = (x.unsqueeze(1) - x.unsqueeze(2)).abs().sum((1, 2)) / (2 * M * (M - 1))   # every pair twice
    crps = ((skill - pair) * wc).sum((1, 2))
    return weight.reshape(()) * crps.sum(), crps.detach()


def eval_metrics(pred, target, pred_std, var_std, interior_weight, kind, map_steps=(), want_mae=False, want_std=False):
    """The evaluation tensors of ``validation_step`` / ``test_step`` (models/module.py:491-504, :546-576, :607-681) in one pass
    over the rollout and a fixed-order reduction (nlam_eval_metrics): no autograd, no host synchronisation (capturable).

    pred, target (B, T, N, F) fp32; pred_std (B, T, N, F) per-entry std (bf16 / fp16 under autocast is widened) or None;
    var_std (F,) the per-variable std, read when pred_std is None (mse / mae read neither); interior_weight (N,) = interior /
    #interior; kind a ``_lib.LOSS_*`` value or its name; map_steps 0-based lead times < T of the loss maps.  Returns a dict of
    device tensors: ``step_loss`` (B, T) and ``sq`` (B, T, F) always, ``ab`` (B, T, F) with ``want_mae``, ``std_mean`` (B, T, F)
    with ``want_std`` (needs pred_std), ``maps`` (B, len(map_steps), N) when map_steps is not empty (NaN off the interior)."""
    lib = L.load()
    if isinstance(kind, str):
        if kind.lower() not in L.LOSS_KINDS:
            raise ValueError(f"eval_metrics: unknown loss kind {kind!r}")
        kind = L.LOSS_KINDS[kind.lower()]
    if kind not in L.LOSS_KINDS.values():
        raise ValueError(f"eval_metrics: unknown loss kind {kind!r}")
    if pred.dim() != 4 or target.shape != pred.shape:
        raise ValueError(f"eval_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} must both be (B, T, N, F)")
    B, T, N, F = pred.shape
    if pred_std is not None and pred_std.dtype in (torch.bfloat16, torch.float16):
        pred_std = pred_std.float()   # an output_std head under autocast
    reads_std = kind not in (L.LOSS_MSE, L.LOSS_MAE)
    std = pred_std if (reads_std or want_std) else None
    vstd = var_std if (reads_std and std is None) else None
    if reads_std and std is None and vstd is None:
        raise ValueError("eval_metrics: this loss kind needs pred_std or var_std")
    if want_std and pred_std is None:
        raise ValueError("eval_metrics: want_std needs a per-entry pred_std")
    checks = [("pred", pred, (B, T, N, F)), ("target", target, (B, T, N, F)), ("interior_weight", interior_weight, (N,))]
    if std is not None:
        checks.append(("pred_std", std, (B, T, N, F)))
    if vstd is not None:
        checks.append(("var_std", vstd, (F,)))
    for name, t, shape in checks:
        if not t.is_cuda or t.device != pred.device:
            raise ValueError(f"eval_metrics: {name} must be on the GPU of pred ({pred.device}), got {t.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"eval_metrics: {name} must be fp32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"eval_metrics: {name} must be contiguous")
        if tuple(t.shape) != shape:
            raise ValueError(f"eval_metrics: {name} has shape {tuple(t.shape)}, expected {shape}")
    if F > L.EVAL_MAX_VARS:
        raise ValueError(f"eval_metrics: at most {L.EVAL_MAX_VARS} variables, got {F}")
    map_steps = [int(s) for s in map_steps]
    if len(map_steps) > L.EVAL_MAX_MAPS or any(s < 0 or s >= T for s in map_steps):
        raise ValueError(f"eval_metrics: map_steps {map_steps} must be at most {L.EVAL_MAX_MAPS} lead times in [0, {T})")
    dev = pred.device
    nws = int(lib.nlam_eval_workspace_floats(B, T, N, F))
    workspace = torch.empty((nws,), device=dev, dtype=torch.float32)
    out = {"step_loss": torch.empty((B, T), device=dev, dtype=torch.float32),
           "sq": torch.empty((B, T, F), device=dev, dtype=torch.float32)}
    if want_mae:
        out["ab"] = torch.empty((B, T, F), device=dev, dtype=torch.float32)
    if want_std:
        out["std_mean"] = torch.empty((B, T, F), device=dev, dtype=torch.float32)
    if map_steps:
        out["maps"] = torch.empty((B, len(map_steps), N), device=dev, dtype=torch.float32)
    p = L.Eval()
    p.pred, p.target, p.std, p.var_std, p.row_weight = _ptr(pred), _ptr(target), _ptr(std), _ptr(vstd), _ptr(interior_weight)
    p.workspace, p.workspace_floats = _ptr(workspace), nws
    p.step_loss, p.sq, p.ab, p.std_mean, p.maps = (_ptr(out.get(k)) for k in ("step_loss", "sq", "ab", "std_mean", "maps"))
    p.batch, p.steps, p.nodes, p.nvars, p.kind, p.nmaps = B, T, N, F, kind, len(map_steps)
    for i, s in enumerate(map_steps):
        p.map_steps[i] = s
    L.check(lib.nlam_eval_metrics(C.byref(p), _stream()), "nlam_eval_metrics")
    return out


class ConcatFunction(torch.autograd.Function):
    """``torch.cat(sources, dim=-1)`` of (B, N, w_k) rows in one launch (nlam_concat); a stride-0 batch (expand_to_batch)
    is read in place.  Backward: column slices of the incoming gradient (views)."""

    @staticmethod
    def forward(ctx, *srcs):
        lib = L.load()
        _require_gpu(*srcs)
        assert 1 <= len(srcs) <= 6
        p = L.Cat()
        keep = []
        B = max(s.shape[0] for s in srcs)
        N = srcs[0].shape[-2]
        widths = []
        for k, s_ in enumerate(srcs):
            t, b_, bstride, _ = as_batched(s_)
            if b_ not in (1, B) or s_.shape[-2] != N:
                raise RuntimeError("concat: inconsistent batch / row counts")
            keep.append(t)
            p.ptr[k], p.bstride[k], p.width[k] = t.data_ptr(), (bstride if b_ == B and B > 1 else 0), s_.shape[-1]
            widths.append(s_.shape[-1])
        out = torch.empty((B, N, sum(widths)), device=srcs[0].device, dtype=torch.float32)
        p.nsrc, p.batch, p.nodes, p.out = len(srcs), B, N, _ptr(out)
        L.check(lib.nlam_concat(C.byref(p), _stream()), "nlam_concat")
        ctx.widths = widths
        ctx.shapes = [tuple(s_.shape) for s_ in srcs]
        return out

    @staticmethod
    def backward(ctx, g):
        grads, off = [], 0
        for k, w in enumerate(ctx.widths):
            gk = None
            if ctx.needs_input_grad[k]:
                gk = g[..., off : off + w]
                if gk.shape != ctx.shapes[k]:   # a broadcast source
                    gk = gk.sum(0, keepdim=True).expand(ctx.shapes[k]) if len(ctx.shapes[k]) == g.dim() else gk.sum(0)
            grads.append(gk)
            off += w
        return tuple(grads)


class CatMLPFunction(torch.autograd.Function):
    """``mlp(torch.cat(pieces, dim=-1))`` with the concatenation folded into the MLP's first load (nlam_mlp_fwd with cat
    pieces): the grid input features in front of ``grid_embedder`` (step_predictors/graph/base.py:275-286) -- previous
    state, state before that, forcing window, static features -- are read straight from their own tensors (the static
    features un-expanded), so the (B, N, 56) tensor exists only as a by-product the kernel writes in training mode for the
    weight gradient and the backward pass.  Shapes the piece path does not serve (fp32 matrix mode, > 64 columns) fall back
    to nlam_concat + the plain launch inside this Function.

    forward(W1, b1, W2, b2, ln_w, ln_b, *pieces (B | expanded, N, w_k)) -> (B, N, dout)"""

    @staticmethod
    def forward(ctx, W1, b1, W2, b2, ln_w, ln_b, *pieces):
        lib = L.load()
        mm_flags = _mm_flags()
        pieces = tuple(x if x.dtype == torch.float32 else x.float() for x in pieces)
        _require_gpu(W1, b1, W2, b2, ln_w, ln_b, *pieces)
        if not 1 <= len(pieces) <= L.NLAM_MAX_CAT or any(x.dim() != 3 for x in pieces):
            raise RuntimeError("CatMLPFunction: 1..6 pieces of shape (B, N, w)")
        hid, kin = W1.shape
        dout = W2.shape[0]
        binfo = [as_batched(x) for x in pieces]
        B = max(bi[1] for bi in binfo)
        N = pieces[0].shape[-2]
        widths = [x.shape[-1] for x in pieces]
        if sum(widths) != kin or any(x.shape[-2] != N for x in pieces) or any(bi[1] not in (1, B) for bi in binfo):
            raise RuntimeError(f"CatMLPFunction: pieces {[tuple(x.shape) for x in pieces]} do not concatenate to (B, N, {kin})")
        dev = pieces[0].device
        need_grad = any(ctx.needs_input_grad)
        p = L.MlpFwd()
        p.nsrc, p.batch, p.rows, p.ntiles = 1, B, N, (N + 31) // 32
        p.src[0].width, p.src[0].bstride = kin, N * kin
        p.ncat = len(pieces)
        for k, (t, b_, bstride, _) in enumerate(binfo):
            p.cat_ptr[k], p.cat_bstride[k], p.cat_width[k] = t.data_ptr(), (bstride if b_ == B and B > 1 else 0), widths[k]
        W1c, b1c, W2c, b2c = W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()
        p.W1, p.b1, p.W2, p.b2, p.ln_w, p.ln_b = _ptr(W1c), _ptr(b1c), _ptr(W2c), _ptr(b2c), _ptr(ln_w), _ptr(ln_b)
        p.eps, p.hid, p.dout, p.flags = 1e-5, hid, dout, mm_flags
        out = torch.empty((B, N, dout), device=dev, dtype=torch.float32)
        p.out, p.out_bstride = _ptr(out), N * dout
        catbuf = z1 = xhat = rstd = None
        if need_grad:
            catbuf = torch.empty((B, N, kin), device=dev, dtype=torch.float32)
            p.cat_out = _ptr(catbuf)
            z1 = torch.empty((B, N, hid), device=dev, dtype=torch.float32)
            p.z1 = _ptr(z1)
            if ln_w is not None:
                xhat = torch.empty((B, N, dout), device=dev, dtype=torch.float32)
                rstd = torch.empty((B, N), device=dev, dtype=torch.float32)
                p.xhat, p.rstd = _ptr(xhat), _ptr(rstd)
        pack = None
        gemm = uses_gemm_family(hid, dout, [kin])   # above the fused widths: concatenation, then the tiled-GEMM family
        wide = gemm or lib.nlam_mlp_fwd_wpack_floats(C.byref(p)) > 0
        if not wide and PACKER is not None:
            pack = PACKER.get(W1c, W2c, [kin], hid, dout, False, 0, mm_flags)
            if pack is not None:
                p.wpack, p.wpack_floats = pack.fwd.data_ptr(), pack.fwd.numel()
        key = ("mlp_fwd", N * B, kin, hid, dout, 1, False, need_grad)

        def meta():
            nbytes = sum(x.shape[-2] * w * 4 * (B if bi[2] != 0 or B == 1 else 1) for x, w, bi in zip(pieces, widths, binfo)) + out.numel() * 4
            nbytes += sum(t_.numel() * 4 for t_ in (catbuf, z1, xhat, rstd) if t_ is not None)
            name, mf = _mm_executed(mm_flags, hid, dout, [kin])
            return {"flops": 2.0 * N * B * (kin * hid + hid * dout), "bytes": float(nbytes), "mm": name, "mfmas_per_block": mf,
                    "what": f"concat of {len(pieces)} pieces folded into Linear-SiLU-Linear" + ("-LayerNorm" if ln_w is not None else "")}

        rc = -2 if wide else PROFILE.launch(key, lambda: lib.nlam_mlp_fwd(C.byref(p), _stream()), meta)
        if rc == -2:   # NLAM_EUNSUP: materialise the concatenation (one launch) and run the plain single-source MLP on it
            q = L.Cat()
            for k, (t, b_, bstride, _) in enumerate(binfo):
                q.ptr[k], q.bstride[k], q.width[k] = t.data_ptr(), (bstride if b_ == B and B > 1 else 0), widths[k]
            if catbuf is None:
                catbuf = torch.empty((B, N, kin), device=dev, dtype=torch.float32)
            q.nsrc, q.batch, q.nodes, q.out = len(pieces), B, N, _ptr(catbuf)
            L.check(lib.nlam_concat(C.byref(q), _stream()), "nlam_concat")
            p.ncat, p.cat_out = 0, None
            _fill_src(p.src[0], catbuf, N * kin, kin, None)
            if gemm:
                nwp = _gemm_ws(lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p)), "nlam_mlp_fwd_gemm_workspace_floats")
            else:
                nwp = lib.nlam_mlp_fwd_wpack_floats(C.byref(p))
            if nwp > 0:
                wpack = torch.empty((nwp,), device=dev, dtype=torch.float32)
                p.wpack, p.wpack_floats = _ptr(wpack), nwp
            rc = (lib.nlam_mlp_fwd_gemm if gemm else lib.nlam_mlp_fwd)(C.byref(p), _stream())
        L.check(rc, "nlam_mlp_fwd (concatenated pieces)")
        if need_grad:
            ctx.geom, ctx.B, ctx.rows, ctx.ntiles = MlpGeometry(nsrc=1), B, N, (N + 31) // 32
            ctx.binfo = [(B, N * kin)]
            ctx.src_shapes = [(B, N, kin)]
            ctx.twin_of = {}
            ctx.has_ln = ln_w is not None
            ctx.param_refs = (W1, b1, W2, b2, ln_w, ln_b)
            ctx.gemm = gemm
            bflags = mm_flags if gemm else _bwd_flags(mm_flags, narrow=not wide)
            ctx.mm_flags, ctx.pack = bflags, _bwd_pack(pack, mm_flags, bflags, W1c, W2c, [kin], hid, dout, False, 0)
            ctx.widths, ctx.piece_shapes = widths, [tuple(x.shape) for x in pieces]
            if GRAD_LISTENER is not None:
                GRAD_LISTENER.note_use([q_ for q_ in ctx.param_refs if q_ is not None and q_.requires_grad])
            ctx.save_for_backward(W1c, W2c, ln_w, z1, xhat, rstd, catbuf)
            ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        npieces = len(ctx.widths)
        if g_out is None:
            return (None,) * (6 + npieces)
        needs = (False, *ctx.needs_input_grad[0:6], any(ctx.needs_input_grad[6:]))
        res = _fused_mlp_backward(ctx, g_out, None, needs)
        g_cat = res[7]
        grads, off = [], 0
        for k, w in enumerate(ctx.widths):
            gk = None
            if ctx.needs_input_grad[6 + k] and g_cat is not None:
                gk = g_cat[..., off : off + w]
                if gk.shape != ctx.piece_shapes[k]:   # a piece shared by the batch (expand_to_batch)
                    gk = gk.sum(0, keepdim=True).expand(ctx.piece_shapes[k])
            grads.append(gk)
            off += w
        return (*res[1:7], *grads)


def standardize(items, outs=None):
    """``ForecasterModule.on_after_batch_transfer`` (models/module.py:326-367) for up to four tensors in one launch.

    items: list of (x, mean, std, rep) -> list of ``(x - mean.repeat_interleave(rep)) / std.repeat_interleave(rep)``
    (fp32, last dim = features).  The batch is data: no autograd.  ``outs``: preallocated outputs (the static inputs of
    a captured step: the standardisation then doubles as the copy of the batch into the graph's buffers)."""
    lib = L.load()
    assert 1 <= len(items) <= 4
    jobs = L.StdJobs()
    given, outs, keep = outs, [], []
    for k, (x, mean, std, rep) in enumerate(items):
        _require_gpu(x, mean, std)
        xc, mc, sc = x.detach().contiguous(), mean.contiguous(), std.contiguous()
        width = xc.shape[-1]
        if width % rep != 0 or mc.numel() * rep != width or sc.numel() != mc.numel():
            raise RuntimeError(f"standardize: {mc.numel()} statistics x window {rep} do not cover {width} features")
        out = torch.empty_like(xc) if given is None else given[k]
        if out.shape != xc.shape or out.dtype != torch.float32 or not out.is_contiguous() or xc.dtype != torch.float32:
            raise RuntimeError(f"standardize: output {tuple(out.shape)} / {out.dtype} does not fit input {tuple(xc.shape)} / {xc.dtype}")
        j = jobs.job[k]
        j.x, j.out, j.mean, j.std = _ptr(xc), _ptr(out), _ptr(mc), _ptr(sc)
        j.rows, j.width, j.rep = (xc.numel() // width if width else 0), width, rep
        outs.append(out)
        keep.extend((xc, mc, sc))
    jobs.njobs = len(items)
    L.check(lib.nlam_standardize(C.byref(jobs), _stream()), "nlam_standardize")
    return outs


class LRSchedule:
    """A closed-form learning-rate schedule that ``AdamWFlat`` evaluates ON THE DEVICE from its resident step count, so a
    captured optimizer stays captured while the rate moves.  ``kind``: ``"constant"``, ``"warmup_cosine"`` or
    ``"warmup_linear"``; ``warmup_steps`` = W, ``total_steps`` = T, ``min_ratio`` = r.  The update after ``s`` earlier
    ones uses ``lr * factor(s)`` -- ``torch.optim.lr_scheduler.LambdaLR(opt, schedule.factor)`` stepped after every
    ``opt.step()``:

        f(s) = (s + 1) / W                        s < W
        p    = min(1, (s - W) / max(1, T - W))    otherwise
        constant 1;  warmup_cosine r + (1 - r) (1 + cos(pi p)) / 2;  warmup_linear r + (1 - r) (1 - p)"""

    KINDS = ("constant", "warmup_cosine", "warmup_linear")

    def __init__(self, kind, warmup_steps=0, total_steps=None, min_ratio=0.0):
        if kind not in self.KINDS:
            raise ValueError(f"unknown schedule {kind!r}: one of {', '.join(self.KINDS)}")
        if int(warmup_steps) != warmup_steps or not 0 <= warmup_steps < 2**31:
            raise ValueError(f"warmup_steps must be a step count, not {warmup_steps!r}")
        if kind != "constant":
            if total_steps is None:
                raise ValueError(f"the {kind!r} schedule needs total_steps")
            if int(total_steps) != total_steps or not 0 <= total_steps < 2**31:
                raise ValueError(f"total_steps must be a step count, not {total_steps!r}")
        if not 0.0 <= float(min_ratio) <= 1.0:
            raise ValueError(f"min_ratio must lie in [0, 1], not {min_ratio!r}")
        fields = dict(kind=kind, warmup_steps=int(warmup_steps), total_steps=None if total_steps is None else int(total_steps),
                      min_ratio=float(min_ratio))
        for k, v in fields.items():
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        # W, T, r and the kind are launch constants of a captured control kernel: a replay would not see a change
        raise AttributeError(f"LRSchedule is immutable (cannot set {name!r}): build a new one and a new optimizer / Trainer")

    def factor(self, s) -> float:
        s, W, r = int(s), self.warmup_steps, self.min_ratio
        if s < W:
            return (s + 1) / W
        if self.kind == "constant":
            return 1.0
        p = min(1.0, (s - W) / max(1, self.total_steps - W))
        if self.kind == "warmup_cosine":
            return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * p))
        return r + (1.0 - r) * (1.0 - p)

    def state_dict(self) -> dict:
        return dict(kind=self.kind, warmup_steps=self.warmup_steps, total_steps=self.total_steps, min_ratio=self.min_ratio)

    def __repr__(self):
        return f"LRSchedule({self.kind!r}, warmup_steps={self.warmup_steps}, total_steps={self.total_steps}, min_ratio={self.min_ratio})"


def global_grad_norm(flat_grad, scale: float = 1.0):
    """``scale * ||flat_grad||_2`` as a 0-dim fp32 device tensor, with no host synchronisation (it can be captured): one
    pass with fp64 sums in a fixed order (``nlam_grad_sumsq``), bit-identical from run to run.  What
    ``torch.nn.utils.clip_grad_norm_`` returns for the one flat gradient of the drop-in path."""
    _require_gpu(flat_grad)
    if flat_grad.dtype != torch.float32 or not flat_grad.is_contiguous():
        raise RuntimeError(f"global_grad_norm: a contiguous fp32 tensor is needed, not {flat_grad.dtype} / strides {flat_grad.stride()}")
    lib = L.load()
    n = flat_grad.numel()
    nws = int(lib.nlam_grad_sumsq_workspace_doubles(n))
    partials = torch.empty((nws,), device=flat_grad.device, dtype=torch.float64)
    norm = torch.empty((), device=flat_grad.device, dtype=torch.float32)
    L.check(lib.nlam_grad_sumsq(_ptr(flat_grad), n, _ptr(partials), nws, float(scale), _ptr(norm), _stream()), "nlam_grad_sumsq")
    return norm


class AdamWFlat:
    """torch.optim.AdamW(lr, betas=(0.9, 0.95)) semantics (models/module.py:293-304)
    on one flat fp32 buffer: a single HBM-bound kernel per step.

    Optimizer controls (all off by default; with none set ``step`` issues exactly the two launches of
    ``nlam_adamw_step_resident``).  With any of them ``step`` is three launches -- the gradient's sum of squares, one wave
    that decides, the update (``nlam_adamw_step_controlled``) -- none of whose arguments depends on the step, so the
    optimizer stays inside a captured graph:

    * ``max_grad_norm``: clip by global norm, ``torch.nn.utils.clip_grad_norm_``'s coefficient, taken from the norm of the
      gradient AFTER the ``grad_scale`` (1 / world) average;
    * ``lr_schedule``: an ``LRSchedule`` evaluated from the resident step count (``lr`` stays the base rate);
    * ``skip_nonfinite``: a step whose gradient norm is inf / nan changes nothing -- parameters, moments, step count and bias
      corrections stay -- and is counted in ``skipped_steps``.  The host mirror ``t`` then counts attempts, not updates:
      ``step_count()`` reads the truth from the device;
    * ``accumulate`` = K > 1 (Lightning's ``accumulate_grad_batches``): a call is one micro-batch and every K-th call
      updates.  The caller does ``begin()``; add its gradient into ``flat_grad``; ``step(grad_scale / K, loss=...)``.  Both ends
      are decided ON THE DEVICE from a block of ``NLAM_ACCUM_WORDS`` words: ``begin()`` zeroes the gradient only in front of
      the first micro-batch of a window, and ``step`` (``nlam_adamw_step_accum``: the same three launches, each gated) holds
      until the last one -- the norm is that of the whole window's gradient.  The launches are the same on every call, so a
      step recorded once serves all of them.  ``micro_step`` is the host mirror of the index within the window, ``t``
      advances on the closing call only, and ``grad_norm`` / ``last_lr`` / ``clip_coef`` keep the last closed window's values
      while a window is open.  A window skipped for a non-finite norm is closed all the same: the next ``begin()`` clears
      the poisoned gradient.

    ``ema_decay`` (off by default): an exponential moving average of the parameters in ``ema``, a flat fp32 copy taken at
    construction -- ``AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay))`` stepped after every optimizer step, started as
    ``EMAWeightAveraging(update_starting_at_step=ema_start_step)`` starts it.  It is written by the update launch itself (the
    ``_ema`` entry of whichever path ``step`` takes: no launch more), from the parameter value that launch holds: untouched
    before applied update ``ema_start_step``, a copy at it, ``ema + (1 - decay) * (p - ema)`` behind it -- and untouched
    wherever the parameters are (a skipped step, a micro-batch inside a window).  It does not make the optimizer
    ``controlled``."""

    def __init__(self, flat_param, flat_grad, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 lr_schedule=None, skip_nonfinite=False, accumulate=1, ema_decay=None, ema_start_step=1):
        self.p, self.g = flat_param, flat_grad
        self.m = torch.zeros_like(flat_param)
        self.v = torch.zeros_like(flat_param)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        # the step count lives on the device (nlam_adamw_step_resident): no launch argument changes from step to step, so the
        # update can be captured into the trainer's HIP graph; ``t`` is the host's mirror of it
        self.t = 0
        self.t_dev = torch.zeros((1,), device=flat_param.device, dtype=torch.int32)
        self.bc_dev = torch.zeros((2,), device=flat_param.device, dtype=torch.float32)
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be positive (or None), not {max_grad_norm!r}")
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise TypeError("lr_schedule must be an ops.LRSchedule (a host-driven scheduler sets opt.lr instead)")
        # launch constants of the control kernel, fixed here (read-only properties below): a captured step carries them
        self._max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._lr_schedule, self._skip_nonfinite = lr_schedule, bool(skip_nonfinite)
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"accumulate must be a count of micro-batches >= 1, not {accumulate!r}")
        self._accumulate = int(accumulate)
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:   # (false for nan)
            raise ValueError(f"ema_decay must lie in [0, 1) (or be None), not {ema_decay!r}")
        if int(ema_start_step) != ema_start_step or ema_start_step < 1:
            raise ValueError(f"ema_start_step must be an update count >= 1, not {ema_start_step!r}")
        self._ema_decay = None if ema_decay is None else float(ema_decay)
        self._ema_start_step = int(ema_start_step)
        self.ema = None if ema_decay is None else flat_param.detach().clone()
        self._controlled = (self._max_grad_norm is not None or lr_schedule is not None or self._skip_nonfinite
                            or self._accumulate > 1)
        self.micro_step = 0   # host mirror of word 0 of ``acc``: calls mod K
        self._window_loss = None
        if self._accumulate > 1:
            # the device block of nlam_accum_t.accum (index in the window, hold flag as words; loss sum, window loss as floats)
            self.acc = torch.zeros((L.ACCUM_WORDS,), device=flat_param.device, dtype=torch.int32)
            self._acc_f = self.acc.view(torch.float32)
        if self.controlled:
            # the device block of nlam_optctl_t.control (lr_t, coefficient, norm as floats; skip flag, skipped steps as words)
            self.ctl = torch.zeros((L.OPTCTL_WORDS,), device=flat_param.device, dtype=torch.int32)
            self._ctl_f = self.ctl.view(torch.float32)
            nws = int(L.load().nlam_grad_sumsq_workspace_doubles(flat_param.numel()))
            self._partials = torch.zeros((nws,), device=flat_param.device, dtype=torch.float64)

    # The controls are chosen at construction and cannot be assigned afterwards: they size the device blocks and are
    # constants of a captured control launch, which a replay would go on using whatever the attribute said.  (``lr``,
    # ``betas``, ``eps`` and ``wd`` stay assignable: the trainer watches those, see ``Trainer._opt_signature``.)
    max_grad_norm = property(lambda self: self._max_grad_norm)
    lr_schedule = property(lambda self: self._lr_schedule)
    skip_nonfinite = property(lambda self: self._skip_nonfinite)
    controlled = property(lambda self: self._controlled)
    accumulate = property(lambda self: self._accumulate)
    ema_decay = property(lambda self: self._ema_decay)
    ema_start_step = property(lambda self: self._ema_start_step)

    def _ema_arg(self):
        """The nlam_ema_t of this optimizer's ``_ema`` launches."""
        e = L.Ema()
        e.ema, e.decay, e.start_step = _ptr(self.ema), self._ema_decay, self._ema_start_step
        return e

    def begin(self):
        """The head of a step, in front of forward + backward: the gradient is zeroed -- with ``accumulate`` > 1 by a launch
        that does so only when the device says a window opens here (``nlam_accum_begin``), so it can be captured."""
        if self._accumulate == 1:
            self.g.zero_()
            return
        L.check(L.load().nlam_accum_begin(_ptr(self.g), self.g.numel(), _ptr(self.acc), _stream()), "nlam_accum_begin")

    def _advance(self):
        self.micro_step = (self.micro_step + 1) % self._accumulate
        if self.micro_step == 0:   # this call closed a window
            self.t += 1

    def step(self, grad_scale: float = 1.0, loss=None):
        """One update (eager or inside a stream capture).  A caller that REPLAYS a captured step calls ``note_replayed``.
        With ``accumulate`` > 1: one micro-batch; ``loss`` (a 0-dim fp32 device tensor) is averaged over the window on the
        device (``window_loss``)."""
        if self._accumulate > 1:
            self._advance()
            return self._step_controlled(grad_scale, loss)
        self.t += 1
        if self.controlled:
            return self._step_controlled(grad_scale)
        args = (_ptr(self.p), _ptr(self.g), _ptr(self.m), _ptr(self.v), self.p.numel(), self.lr, self.betas[0],
                self.betas[1], self.eps, self.wd, _ptr(self.t_dev), _ptr(self.bc_dev), grad_scale, _stream())
        if self.ema is not None:
            L.check(L.load().nlam_adamw_step_resident_ema(*args, C.byref(self._ema_arg())), "nlam_adamw_step_resident_ema")
            return
        L.check(L.load().nlam_adamw_step_resident(*args), "nlam_adamw_step_resident")

    def _optctl(self, grad_scale):
        """The nlam_optctl_t of this optimizer's controlled launches."""
        c, sch = L.OptCtl(), self.lr_schedule
        c.param, c.grad, c.exp_avg, c.exp_avg_sq = _ptr(self.p), _ptr(self.g), _ptr(self.m), _ptr(self.v)
        c.step_count_dev, c.bias_corr_dev = _ptr(self.t_dev), _ptr(self.bc_dev)
        c.partials, c.control = _ptr(self._partials), _ptr(self.ctl)
        c.n, c.partials_doubles = self.p.numel(), self._partials.numel()
        c.lr, c.beta1, c.beta2, c.eps, c.weight_decay, c.grad_scale = self.lr, self.betas[0], self.betas[1], self.eps, self.wd, grad_scale
        c.max_grad_norm = 0.0 if self.max_grad_norm is None else self.max_grad_norm
        if sch is not None:
            c.schedule, c.warmup_steps, c.min_ratio = L.SCHED_KINDS[sch.kind], sch.warmup_steps, sch.min_ratio
            c.total_steps = 0 if sch.total_steps is None else sch.total_steps
        else:
            c.schedule = L.SCHED_NONE
        c.skip_nonfinite = int(self.skip_nonfinite)
        return c

    def _step_controlled(self, grad_scale, loss=None):
        c = self._optctl(grad_scale)
        if self._accumulate == 1:
            if self.ema is not None:
                L.check(L.load().nlam_adamw_step_controlled_ema(C.byref(c), None, C.byref(self._ema_arg()), _stream()),
                        "nlam_adamw_step_controlled_ema")
                return
            L.check(L.load().nlam_adamw_step_controlled(C.byref(c), _stream()), "nlam_adamw_step_controlled")
            return
        a = L.Accum()
        a.accum, a.steps = _ptr(self.acc), self._accumulate
        if loss is not None and loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == self.acc.device:
            a.loss = _ptr(loss)
            self._window_loss = self._acc_f[L.ACCUM_WINDOW_LOSS]
        if self.ema is not None:
            L.check(L.load().nlam_adamw_step_controlled_ema(C.byref(c), C.byref(a), C.byref(self._ema_arg()), _stream()),
                    "nlam_adamw_step_controlled_ema")
            return
        L.check(L.load().nlam_adamw_step_accum(C.byref(c), C.byref(a), _stream()), "nlam_adamw_step_accum")

    @property
    def window_loss(self):
        """The mean of the micro-batch losses of the last closed window: a 0-dim device tensor, read without a synchronise (a
        view of the accumulation block).  Exists once ``step`` has been handed a 0-dim fp32 device loss."""
        if self._window_loss is None:
            raise AttributeError("window_loss exists with accumulate > 1, after a step(..., loss=<0-dim fp32 device tensor>)")
        return self._window_loss

    def reset_window(self):
        """Back to a window boundary (a checkpoint was loaded): the next call is the first micro-batch of a window."""
        self.micro_step = 0
        if self._accumulate > 1:
            self.acc.zero_()

    def _control_word(self, k, as_float):
        if not self.controlled:
            raise AttributeError("grad_norm / last_lr / skipped_steps exist with max_grad_norm, lr_schedule or skip_nonfinite set")
        return (self._ctl_f if as_float else self.ctl)[k]

    @property
    def grad_norm(self):
        """The last step's pre-clip norm of the averaged gradient: a 0-dim device tensor, read without a synchronise (a
        view of the control block: ``clone()`` it to keep a step's value)."""
        return self._control_word(L.OPTCTL_NORM, True)

    @property
    def last_lr(self):
        """The learning rate the last applied update used (device tensor, as ``grad_norm``)."""
        return self._control_word(L.OPTCTL_LR, True)

    @property
    def clip_coef(self):
        """The factor the last step's gradient was multiplied with: 1 unless clipped, 0 for a skipped step."""
        return self._control_word(L.OPTCTL_COEF, True)

    @property
    def skipped_steps(self) -> int:
        """Steps the non-finite guard refused so far (reads the device counter: a synchronise)."""
        return int(self.ctl[L.OPTCTL_SKIPPED].item()) if self.controlled else 0

    def set_skipped_steps(self, n: int):
        """Restore the device counter (checkpoints)."""
        self.ctl[L.OPTCTL_SKIPPED : L.OPTCTL_SKIPPED + 1].fill_(n)

    def step_count(self) -> int:
        """Updates applied so far, from the device (with ``skip_nonfinite`` the mirror ``t`` also counts refused steps)."""
        return int(self.t_dev.item())

    def scheduled_lr(self, t=None) -> float:
        """The rate update ``t + 1`` uses (``t``: updates applied, default ``step_count()``): where a torch scheduler
        stepped after every update leaves ``param_groups[0]["lr"]``."""
        if self.lr_schedule is None:
            return self.lr
        return self.lr * self.lr_schedule.factor(self.step_count() if t is None else t)

    capturable = True

    def note_replayed(self):
        if self._accumulate > 1:
            self._advance()
        else:
            self.t += 1
