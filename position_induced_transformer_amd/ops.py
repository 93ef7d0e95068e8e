"""Host-side operators of the PiT hot path: thin autograd wrappers over the C ABI.

Each wrapper allocates outputs / workspaces with torch (caller-owned memory, see
include/pit_hip.h), launches on torch's current HIP stream and never synchronises, so a
whole training step can be captured into a hipGraph (torch.cuda.graph).  There is no
CPU or eager-PyTorch path: tensors must live on the GPU and the shared library must load.
"""
from __future__ import annotations

import collections
import ctypes
import math
import os
import threading
import types
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from . import _lib

# The header's values this module uses, bound once at import (include/pit_hip.h through _lib.DEFINES): no launch path looks one up
_H = _lib.DEFINES
METRIC_ID = {"euclid": _H["PIT_METRIC_EUCLID"], "periodic1d": _H["PIT_METRIC_PERIODIC1D"], "periodic2d": _H["PIT_METRIC_PERIODIC2D"]}
MAX_SPACE_DIM = _H["PIT_MAX_SPACE_DIM"]                # coordinates per mesh point
MATH_MODES = {"fp32": _H["PIT_MATH_FP32"], "bf16": _H["PIT_MATH_BF16"]}
# bf16 STORAGE flags of the `math_mode` argument
IO_X_BF16, IO_SAVE_BF16, IO_DX_BF16 = _H["PIT_IO_X_BF16"], _H["PIT_IO_SAVE_BF16"], _H["PIT_IO_DX_BF16"]
IO_OUT_BF16, IO_DOUT_BF16 = _H["PIT_IO_OUT_BF16"], _H["PIT_IO_DOUT_BF16"]
ATT_UNION = _H["PIT_ATT_UNION"]
SLAB_UNION_MAX = _H["PIT_SLAB_UNION_MAX"]
LIST_MAX_CAP = _H["PIT_DISTLIST_MAX_CAP"]              # slots of a row the selection holds in registers
KNN_MAX_K = _lib.KNN_MAX_K                             # the width the list layers accept (LIST_MAX_CAP)
KNN_REG_MAX_KEYS = _lib.KNN_REG_MAX_KEYS               # longer rows are streamed (form 2)
_DSCALE_SLOTS = _H["PIT_DSCALE_SLOTS"]                 # fp64 accumulators per head of a d(scale) workspace
_HEAD_ACCUMULATE, _HEAD_DEFER, _HEAD_IS_SCALE = _H["PIT_HEAD_ACCUMULATE"], _H["PIT_HEAD_DEFER"], _H["PIT_HEAD_IS_SCALE"]
_EVAL_ADVANCE, _EVAL_STORE_TRUE = _H["PIT_EVAL_ADVANCE"], _H["PIT_EVAL_STORE_TRUE"]
_ERR_UNSUPPORTED = _H["PIT_ERR_UNSUPPORTED"]
del _H

# In-place gradient accumulation is OPT-IN per parameter: ddp.FlatGradients marks the parameters whose
# ``.grad`` it owns (``mark_inplace_grad``), and only for those - while the ``.grad`` is still the
# registered view and the parameter carries no autograd hooks - the backward kernels accumulate
# straight into ``.grad`` and autograd receives ``None`` for that input (no memset of a temporary,
# no separate ``grad += tmp`` launch).  Every other parameter gets its gradient RETURNED to autograd,
# so tensor hooks, post-accumulate hooks, torch DDP's reducer and ``torch.autograd.grad`` behave as
# with any torch op.  Set to False to disable the in-place path altogether.
FUSED_GRAD_ACCUMULATION = True

# Masked (locality < 1) layers run on per-row candidate lists (O(N*k) work) when the lists are
# much shorter than the key axis; False forces the dense MFMA kernels everywhere.
SPARSE_MASKED = True

_DSCALE_WS = {}     # (device index, stream) -> fp64 accumulators
_LOSS_WS = {}       # (device index, stream) -> loss accumulator + ticket
# Tensors whose addresses were baked into a hipGraph under capture (mesh plans, accumulators): never
# released, so a cache eviction cannot hand their memory to someone else while a graph still replays.
_PINNED = []


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


_PINNED_IDS = set()


def _pin(*objs) -> None:
    for o in objs:
        if id(o) not in _PINNED_IDS:          # (pinned objects are never released, so ids stay unique)
            _PINNED_IDS.add(id(o))
            _PINNED.append(o)


def _ws_key(device):
    return (device.index, torch.cuda.current_stream(device).cuda_stream)


def _graph_task() -> int:
    """Id of the backward pass being executed (-1 outside of one): what the end-of-pass callbacks are
    keyed on, so a pass that died with an exception cannot leave the NEXT pass without its callback."""
    return torch._C._current_graph_task_id()


def _dscale_workspace(device, n_head: int) -> torch.Tensor:
    """fp64 accumulators for d(scale): zero on entry and left zero by pit_posatt_bwd, so one
    zeroed buffer per device serves every layer (launches are stream-ordered)."""
    key = _ws_key(device)                     # per (device, stream): concurrent streams never share accumulators
    ws = _DSCALE_WS.get(key)
    if ws is None or ws.numel() < n_head * _DSCALE_SLOTS + 8:
        ws = torch.zeros(max(8, n_head) * _DSCALE_SLOTS + 8, device=device, dtype=torch.float64)   # slots + counter
        _DSCALE_WS[key] = ws
    if _capturing():
        _pin(ws)
    return ws


# d(lmda) of every attention layer of a backward pass is finished by ONE launch at the end of the
# pass (pit_posatt_dhead_finish) instead of one small kernel per layer; applies when the gradient
# goes in place into lmda.grad (the training path), needs one accumulator buffer per layer.
DEFER_HEAD_FINISH = os.environ.get("PIT_DEFER_HEAD_FINISH", "1") != "0"
# Both this table and the postponed weight-gradient jobs below are keyed on autograd's graph-task id: backward passes
# of DIFFERENT models may interleave (two Python threads calling backward(): the engine's one device thread runs their
# nodes alternately) without seeing each other's entries.  An entry whose pass raised before its end-of-pass callback
# ran is recognised when another pass wants the same accumulators / gradient slots (two live passes accumulating
# into the same .grad are a race in torch itself): its partial sums are zeroed and it is forgotten.
_PENDING_HEADS = {}      # graph-task id -> [(workspace, d_head, lmda, scale, n_head, flags), ...]
_LAYER_WS = {}
_MAX_PENDING_TASKS = 64


def _layer_workspace(slot: torch.Tensor, n_head: int) -> torch.Tensor:
    key = (slot.device.index, slot.data_ptr(), n_head)
    ws = _LAYER_WS.get(key)
    if ws is None:
        while len(_LAYER_WS) >= 1024:         # gradient buffers were re-created many times: drop the oldest
            _LAYER_WS.pop(next(iter(_LAYER_WS)))
        ws = _LAYER_WS[key] = torch.zeros(n_head * _DSCALE_SLOTS, device=slot.device, dtype=torch.float64)
    if _capturing():
        _pin(ws)
    return ws


def _flush_head_finishes(task: int) -> None:
    """End-of-backward callback of graph task ``task``: one launch finishing d(lmda) of all its deferred layers."""
    # a layer applied several times in one pass (the autoregressive rollout: train_vorticity.py:122-126)
    # deferred once per application into the SAME accumulators: drain them once - duplicates in one batch
    # would race on the non-atomic "d_head += ..." of the finishing kernel
    seen, pend = set(), []
    for entry in _PENDING_HEADS.pop(task, ()):
        key = (entry[0].data_ptr(), entry[1].data_ptr())
        if key not in seen:
            seen.add(key)
            pend.append(entry)
    # a weight-gradient job the pass still holds (the encoder MLP's: its fused backward is the pass's last launch, nobody is left
    # to carry it) rides in the finishing launch when it sits on the same device and stream
    job = _PENDING_DW.get(task)
    for dev in sorted({p[0].device.index for p in pend}):
        grp = [p for p in pend if p[0].device.index == dev]
        for i in range(0, len(grp), 32):
            part = grp[i:i + 32]
            rider = None
            if job is not None and job[2].device.index == dev and job[2] == torch.cuda.current_stream(job[2].device):
                rider, job = job, None
                _PENDING_DW[task] = None
            # the jobs the last block launches of a fused processor gave up (_PENDING_TAIL), when they sit on this device and stream
            tail = _tail_take(task, dev)
            with torch.cuda.device(dev):
                _launch_head_finishes(part, rider, tail)


def _launch_head_finishes(entries, rider=None, tail=()) -> None:
    """ONE pit_posatt_dhead_finish launch on the current device and stream: d(lmda) of every layer in ``entries`` =
    [(work, d_head, head, scale, n_head, flags), ...] from its accumulators ``work`` (flags: PIT_HEAD_ACCUMULATE = add into d_head in
    place, PIT_HEAD_IS_SCALE = the head is the scale itself), with the postponed weight-gradient job ``rider`` (_PENDING_DW's form)
    riding along and the jobs ``tail`` (_PENDING_TAIL's form) staged for it (pit_posatt_dhead_finish_stage copies the structs)."""
    if tail:
        jobs = (ctypes.c_void_p * len(tail))(*[ctypes.addressof(t[0]) for t in tail])
        _lib.check(_lib.lib().pit_posatt_dhead_finish_stage(jobs, len(tail)), "pit_posatt_dhead_finish_stage")
    n = len(entries)
    ws, dh, hd, sc = ((ctypes.c_void_p * n)(*[_lib.ptr(e[i]) for e in entries]) for i in range(4))
    nh = (ctypes.c_int * n)(*[e[4] for e in entries])
    fl = (ctypes.c_int * n)(*[e[5] for e in entries])
    rc = _lib.lib().pit_posatt_dhead_finish(n, ws, dh, hd, sc, nh, fl,
                                            ctypes.cast(ctypes.pointer(rider[0]), ctypes.c_void_p) if rider is not None else None,
                                            _lib.stream_ptr())
    _lib.check(rc, "pit_posatt_dhead_finish")


def _finish_heads_now(work, d_head, head, scale, n_head: int, flags: int) -> None:
    """d(lmda) of ONE layer from freshly loaded accumulators, now."""
    _launch_head_finishes([(work, d_head, head, scale, n_head, flags)])


def _defer_head_begin(work: torch.Tensor) -> None:
    """Call BEFORE the backward kernel of a deferred layer loads its accumulators ``work``.  Entries of ANOTHER pass
    on the same accumulators mean that pass raised before its end-of-pass callback ran (autograd skips the
    callbacks then): they hold partial sums of an aborted pass - zero them, forget the entries.  On the first
    deferred layer of this pass: queue its flush."""
    task = _graph_task()
    ptr = work.data_ptr()
    for other in [t for t in _PENDING_HEADS if t != task]:
        stale = [e for e in _PENDING_HEADS[other] if e[0].data_ptr() == ptr]
        if stale:
            stale[0][0].zero_()
            _PENDING_HEADS[other] = [e for e in _PENDING_HEADS[other] if e[0].data_ptr() != ptr]
            if not _PENDING_HEADS[other]:
                del _PENDING_HEADS[other]
    if task not in _PENDING_HEADS:
        while len(_PENDING_HEADS) >= _MAX_PENDING_TASKS:      # passes that died long ago and whose layers never ran again
            for e in _PENDING_HEADS.pop(next(iter(_PENDING_HEADS))):
                e[0].zero_()
        _PENDING_HEADS[task] = []
        torch.autograd.Variable._execution_engine.queue_callback(lambda: _flush_head_finishes(task))


def _defer_head_finish(work, d_head, head, scale, n_head: int, flags: int) -> None:
    _defer_head_begin(work)
    _PENDING_HEADS[_graph_task()].append((work, d_head, head, scale, n_head, flags))


class _HeadGrad:
    """Where ONE attention layer's d(lmda) goes, decided BEFORE the layer's backward launch (which adds d(scale) partial sums into
    ``work``) and carried out by ``finish`` after it:
      returned   lmda did not opt in (_grad_slot): ``d_head`` is a fresh tensor, finished now, handed to autograd;
      in place   ``d_head`` is lmda.grad itself (``slot``), finished now, autograd gets None;
      deferred   in place under DEFER_HEAD_FINISH: the layer's own accumulators (_layer_workspace), finished by the pass's ONE
                 finishing launch (_flush_head_finishes); constructing the object performs _defer_head_begin.
    What differs between the nodes is spelled at their call:
      shared_workspace     the not-deferred accumulators are the stream's _dscale_workspace, which the kernels leave zeroed and
                           which exists whether or not lmda needs a gradient (_PosAtt); otherwise a fresh torch.zeros buffer;
      always_accumulators  accumulators although ``need`` is false: the launch reduces d(scale) unconditionally (_Encoder);
      kernel_finishes      the launch itself forms d(lmda) unless deferred (_PosAtt's candidate-list / dense launch): it is handed
                           ``d_head`` and ``acc`` (PIT_HEAD_ACCUMULATE: add in place, PIT_HEAD_DEFER) and ``finish`` only queues."""
    __slots__ = ("need", "n_head", "scale_bit", "kernel_finishes", "slot", "defer", "work", "d_head")

    def __init__(self, head_param, need: bool, n_head: int, device, head_is_scale: bool, *, shared_workspace: bool = False,
                 always_accumulators: bool = False, kernel_finishes: bool = False):
        self.need, self.n_head, self.kernel_finishes = bool(need), n_head, kernel_finishes
        self.scale_bit = _HEAD_IS_SCALE if head_is_scale else 0
        self.slot = _grad_slot(head_param) if need else None
        self.defer = bool(DEFER_HEAD_FINISH and self.slot is not None)
        if self.defer:
            self.work = _layer_workspace(self.slot, n_head)
            _defer_head_begin(self.work)            # (clears what an aborted pass left, before the kernel adds)
        elif shared_workspace:
            self.work = _dscale_workspace(device, n_head)
        elif need or always_accumulators:
            self.work = torch.zeros(n_head * _DSCALE_SLOTS, device=device, dtype=torch.float64)
        else:
            self.work = None
        if self.slot is not None:
            self.d_head = self.slot                 # accumulate into lmda.grad in place
        else:
            self.d_head = torch.empty((n_head,), device=device, dtype=torch.float32) if need else None

    @property
    def acc(self) -> int:
        return (_HEAD_ACCUMULATE if self.slot is not None else 0) | (_HEAD_DEFER if self.defer else 0)

    def finish(self, head, scale):
        """After the launch: what the backward returns to autograd for lmda (None: not wanted, or it went in place)."""
        return _HeadGrad.finish_all([(self, head, scale)])[0]

    @staticmethod
    def finish_all(layers):
        """``finish`` for [(_HeadGrad, head, scale), ...] of one node: the deferred layers are queued, all others share ONE launch."""
        now = []
        for g, head, scale in layers:
            entry = (g.work, g.d_head, head, scale, g.n_head, (_HEAD_ACCUMULATE if g.slot is not None else 0) | g.scale_bit)
            if g.defer:
                _defer_head_finish(*entry)
            elif g.need and not g.kernel_finishes:
                now.append(entry)
        if now:
            _launch_head_finishes(now)
        return [None if g.slot is not None else g.d_head for g, _, _ in layers]


# The weight-gradient reductions of an MLP backward (dW2|db2, dW1|db1: nothing downstream in the pass reads
# them) are postponed and handed to the NEXT attention backward as its `rider` (pit_hip.h): pit.py:116-121
# runs mlp -> attention, so in the backward the attention launch that consumes the MLP's d_x can carry the
# MLP's reductions along - three small latency-bound grids in one launch.  In-place gradient mode only.
MLP_PARAMS_RIDER = os.environ.get("PIT_DW_RIDER", "1") != "0"
# Per-THREAD step state (round 4; was module-global and toggled per step: two TrainSteps on two threads raced on it).
# engine.TrainStep sets it around its forward; the autograd nodes read it in their FORWARD (which runs on the calling
# thread) and keep it on their ctx - the backward runs on autograd's device thread, where a thread-local of the caller
# is not visible.  `processor_hook`: see _Processor.
_STEP = threading.local()


def _processor_hook():
    return getattr(_STEP, "processor_hook", None)


class step_state:
    """Context manager: per-thread overrides for the autograd nodes built inside it (engine.TrainStep._step)."""

    def __init__(self, processor_hook=None, loss=None, clear=None):
        """``loss``: a LossSpec the step will apply to the model's prediction (the fused decoder takes it); ``clear``: a contiguous
        fp32 tensor the step wants zeroed before its backward (the flat gradient buffer: the fused encoder launch clears it on
        the way).  Whoever takes either resets it to None; what is left when the forward returns is the caller's to do."""
        self.new = (processor_hook, loss, clear)

    def __enter__(self):
        self.old = (getattr(_STEP, "processor_hook", None), getattr(_STEP, "loss", None), getattr(_STEP, "clear", None),
                    getattr(_STEP, "loss_issued", None))
        _STEP.processor_hook, _STEP.loss, _STEP.clear = self.new
        _STEP.loss_issued = None
        return self

    def __exit__(self, *exc):
        _STEP.processor_hook, _STEP.loss, _STEP.clear, _STEP.loss_issued = self.old
        return False


def take_pending_clear():
    """The buffer step_state(clear=...) asked to have zeroed, if no launch of the forward took it (then the caller zeroes it)."""
    t = getattr(_STEP, "clear", None)
    _STEP.clear = None
    return t


_PENDING_DW = {}          # graph-task id -> job = (MlpParamsJob, keep-alive tensors, stream it was prepared on) or None
_DEFERRABLE = {}


def _dw_run(job) -> None:
    """Perform a postponed pit_mlp_bwd_params on the stream its inputs were produced on."""
    st, keep, stream = job
    cur = torch.cuda.current_stream(stream.device)
    with torch.cuda.stream(stream):
        rc = _lib.lib().pit_mlp_bwd_params(st.x, st.ldx, st.rows, st.n0, st.n1, st.n2, st.h, st.out_gelu, st.d_y,
                                           st.ld_dy, st.d_w1, st.d_b1, st.d_w2, st.d_b2, st.accumulate, st.scratch,
                                           st.math_mode, stream.cuda_stream)
    _lib.check(rc, "pit_mlp_bwd_params")
    if cur != stream:
        cur.wait_stream(stream)


def _dw_flush(task: int) -> None:
    """A second MLP backward of the pass with no attention in between (and the end of the pass)."""
    job = _PENDING_DW.get(task)
    if job is not None:
        _PENDING_DW[task] = None
        _dw_run(job)


def _dw_end_of_pass(task: int) -> None:
    _dw_flush(task)
    _PENDING_DW.pop(task, None)


def _dw_defer(st, keep, device) -> None:
    task = _graph_task()
    # a job ANOTHER pass left for the same gradient slots: that pass raised before its end-of-pass callback ran - its
    # gradients are void (two live passes accumulating into one .grad would be a race in torch itself)
    for other in [t for t, j in _PENDING_DW.items() if t != task and j is not None and j[0].d_w1 == st.d_w1]:
        del _PENDING_DW[other]
    if task not in _PENDING_DW:
        while len(_PENDING_DW) >= _MAX_PENDING_TASKS:         # entries of passes that died long ago
            del _PENDING_DW[next(iter(_PENDING_DW))]
        _PENDING_DW[task] = None
        torch.autograd.Variable._execution_engine.queue_callback(lambda: _dw_end_of_pass(task))
    else:
        _dw_flush(task)
    _PENDING_DW[task] = (st, keep, torch.cuda.current_stream(device))


def _dw_take(device):
    """The job the current attention backward should carry (None if there is none for this pass / stream)."""
    task = _graph_task()
    job = _PENDING_DW.get(task)
    if job is None:
        return None
    if job[2] != torch.cuda.current_stream(device):
        _dw_flush(task)                           # produced on another stream: run it there
        return None
    _PENDING_DW[task] = None
    return job


def _dw_run_pending(device) -> None:
    """For a backward whose launch carries no rider: the job the pass has postponed, if any, is performed now."""
    job = _dw_take(device)
    if job is not None:
        _dw_run(job)


# Round 10: the last launches of a fused processor's backward carry no rider (RIDER_TAIL_BLOCKS below); their jobs wait here for the
# pass's finishing launch, which has the compute units and pays the latency of a rider tile anyway.  A table of its own: the
# single slot of _PENDING_DW is flushed by whoever defers next (the encoder) and must be empty when the pass ends.
_PENDING_TAIL = {}        # graph-task id -> [(MlpParamsJob, keep-alive tensors, stream it was prepared on), ...]


def _at_end_of_pass(fn) -> None:
    """Queue ``fn`` behind the running backward pass (autograd runs the callbacks in the order they were queued)."""
    torch.autograd.Variable._execution_engine.queue_callback(fn)


def _tail_defer(jobs) -> None:
    """Hand ``jobs`` (_PENDING_DW's form) to the end of the running pass: the finishing launch stages them (_flush_head_finishes),
    else the end-of-pass callback queued here performs them - whichever runs first takes them out of the table."""
    task = _graph_task()
    if task not in _PENDING_TAIL:
        while len(_PENDING_TAIL) >= _MAX_PENDING_TASKS:       # entries of passes that died long ago (their gradients are void)
            del _PENDING_TAIL[next(iter(_PENDING_TAIL))]
        _PENDING_TAIL[task] = []
        _at_end_of_pass(lambda: _tail_end_of_pass(task))
    _PENDING_TAIL[task].extend(jobs)


def _tail_take(task: int, dev: int) -> list:
    """The pass's tail jobs prepared on device ``dev``'s current stream, removed from the table (the others stay for the callback)."""
    jobs = _PENDING_TAIL.get(task)
    if not jobs:
        return []
    take = [j for j in jobs if j[2].device.index == dev and j[2] == torch.cuda.current_stream(j[2].device)]
    _PENDING_TAIL[task] = [j for j in jobs if not any(j is t for t in take)]
    return take


def _tail_end_of_pass(task: int) -> None:
    """A pass that ended without a finishing launch on the jobs' device and stream: each on its own, where it was prepared."""
    for job in _PENDING_TAIL.pop(task, ()):
        _dw_run(job)


# PIT_RIDER_TAIL_BLOCKS = k: the last k pit_block_bwd launches of a fused processor (blocks k-1 .. 0) carry no rider - their own
# MLP's job and their slice of the decoder MLP's go to the finishing launch.  Read once; tests set the attribute.
RIDER_TAIL_BLOCKS = int(os.environ.get("PIT_RIDER_TAIL_BLOCKS", "1"))


def rider_tail_schedule(n_blocks: int, k: int, complete_by=None, reproducible: bool = False, inplace: bool = True,
                        heads_deferred: bool = True, has_slices: bool = True, chain_fits: bool = True):
    """Which launch of a fused processor's backward carries which weight-gradient job - a pure function.
    ``k`` = RIDER_TAIL_BLOCKS, clamped to [0, n_blocks] and forced to 0 where the jobs cannot wait for the end of the pass: a
    two-bucket step (``complete_by`` = the block by whose launch the decoder MLP's slices must be enqueued: _Processor's hook),
    the reproducible mode, gradients returned to autograd instead of accumulated in place, and a pass whose d(lmda) is not
    deferred (no finishing launch will come).  ``chain_fits`` = the launch's chain and d(scale) workgroups number at most the
    compute units: the one regime the switch was measured in (Darcy b=8) - beyond it k is 0 as well.  Returns (k, n_slices, plan): the postponed decoder job is cut into ``n_slices``
    row slices (0 without one), and plan[j] = (own, slice) for the j-th launch (block n_blocks - 1 - j): where the block's own job
    and slice j go - "launch" (this launch's rider / rider2), "tail" (the finishing launch) or None (no slice j)."""
    n = int(n_blocks)
    k = max(0, min(int(k), n))
    if complete_by is not None or reproducible or not inplace or not heads_deferred or not chain_fits:
        k = 0
    n_slices = 0 if not has_slices else (n if complete_by is None else max(1, n - int(complete_by)))
    plan = []
    for j in range(n):
        where = "tail" if j >= n - k else "launch"
        plan.append((where, where if j < n_slices else None))
    return k, n_slices, plan


_CU_COUNT = {}


def _cu_count(device) -> int:
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    return _CU_COUNT[idx]


BIG_RIDER_ROWS = 8192


def _dw_pending_rows(device) -> int:
    """Rows of the job the running pass has postponed (0: none)."""
    job = _PENDING_DW.get(_graph_task())
    return int(job[0].rows) if job is not None else 0


def _dw_slices(job, parts: int):
    """``job`` (a postponed pit_mlp_bwd_params without trailing gelu: its reductions are plain row sums) cut into
    ``parts`` row slices, each a job of its own with accumulate = 1."""
    st = job[0]
    out, per = [], -(-st.rows // parts // 16) * 16
    for r0 in range(0, st.rows, per):
        n = min(per, st.rows - r0)
        out.append(_lib.MlpParamsJob(st.x + 4 * r0 * st.ldx, st.ldx, n, st.n0, st.n1, st.n2, st.h + 4 * r0 * st.n1, 0,
                                     st.d_y + 4 * r0 * st.ld_dy, st.ld_dy, st.d_w1, st.d_b1, st.d_w2, st.d_b2, 1,
                                     st.scratch + 4 * r0 * st.n1, st.math_mode))
    return out


def _dw_deferrable(rows: int, n0: int, n1: int, n2: int, out_gelu: int, ld_dy: int) -> bool:
    key = (rows, n0, n1, n2, out_gelu, ld_dy)
    v = _DEFERRABLE.get(key)
    if v is None:
        if len(_DEFERRABLE) > 4096:
            _DEFERRABLE.clear()
        v = _DEFERRABLE[key] = bool(_lib.lib().pit_mlp_bwd_params_deferrable(*key))
    return v


def mark_inplace_grad(param, grad_view) -> None:
    """Opt ``param`` in to in-place gradient accumulation into ``grad_view`` (ddp.FlatGradients)."""
    param._pit_grad_ptr = grad_view.data_ptr()


def _grad_slot(param) -> Optional[torch.Tensor]:
    """The parameter's own .grad if the kernels may accumulate into it in place."""
    if not FUSED_GRAD_ACCUMULATION or param is None:
        return None
    want = getattr(param, "_pit_grad_ptr", None)
    g = getattr(param, "grad", None)
    if want is None or g is None or g.data_ptr() != want:
        return None                      # not opted in, or .grad was dropped / replaced (zero_grad(set_to_none=True))
    if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
        return None
    if param._backward_hooks or getattr(param, "_post_accumulate_grad_hooks", None):
        return None                      # hooks must see the gradient: return it to autograd
    return g


def _mlp_grad_slots(params, shapes, needs, device, fresh: str = "zeros"):
    """([d_w1, d_b1, d_w2, d_b2], in place?) for an MLP's weight gradients: the parameters' own .grad (the kernels accumulate) when
    every one of them opted in and needs a gradient, else fresh tensors returned to autograd - ``fresh`` = "zeros": zeroed, the
    kernels add into them (accumulate = 1); "empty": uninitialised, the kernels overwrite them (accumulate = 0: _Mlp)."""
    slots = [_grad_slot(p) if isinstance(p, torch.nn.Parameter) else None for p in params]
    if all(s is not None for s in slots) and all(needs):
        return slots, True
    new = torch.zeros if fresh == "zeros" else torch.empty
    return [new(tuple(sh), device=device, dtype=torch.float32) for sh in shapes], False


def _params_job(x, h, d_y, scratch, grads, dims, out_gelu: int, math: int, ld_dy=None):
    """(MlpParamsJob, the tensors it points into) of an MLP's weight-gradient reductions (pit_mlp_bwd_params' argument list):
    ``x`` (rows, n0) and ``h`` (rows, n1) the forward's operands, ``d_y`` the output gradient with row stride ``ld_dy``, ``scratch``
    the data path's dZ1 (| dZ2), ``grads`` = (d_w1, d_b1, d_w2, d_b2) which it adds to, ``dims`` = (rows, n0, n1, n2)."""
    d_w1, d_b1, d_w2, d_b2 = grads
    st = _lib.MlpParamsJob(x.data_ptr(), x.stride(-2), *dims, h.data_ptr(), out_gelu, d_y.data_ptr(),
                           d_y.stride(0) if ld_dy is None else ld_dy, d_w1.data_ptr(), d_b1.data_ptr(), d_w2.data_ptr(),
                           d_b2.data_ptr(), 1, scratch.data_ptr(), math)
    return st, (x, h, d_y, scratch, d_w1, d_b1, d_w2, d_b2)


def _dw_deliver(job, inplace: bool, device):
    """The weight-gradient tail of a fused edge node: ``job`` (_params_job) is postponed and carried by a later launch of the pass
    in the in-place mode, performed now otherwise; returns the four gradients for autograd (None each when they went in place)."""
    st, keep = job
    if inplace and MLP_PARAMS_RIDER and _dw_deferrable(st.rows, st.n0, st.n1, st.n2, st.out_gelu, st.ld_dy):
        _dw_defer(st, keep, device)
    else:
        _dw_run((st, keep, torch.cuda.current_stream(device)))
    return (None,) * 4 if inplace else tuple(keep[4:])


# bf16 mode: the decoder tail (up-projection output, the decoder MLP's saved activations, their gradients) is kept in
# memory as bf16 when the shapes take the kernels that implement it (pit.decoder asks); PIT_BF16_STORAGE=0: fp32 tensors
BF16_STORAGE = os.environ.get("PIT_BF16_STORAGE", "1") != "0"


def mlp_bf16_io_supported(rows: int, n0: int, n1: int, n2: int) -> bool:
    return BF16_STORAGE and get_math_mode() == "bf16" and bool(_lib.lib().pit_mlp_bf16_io_supported(rows, n0, n1, n2, 0))


def _need_gpu_bf16_ok(t) -> None:
    if t is not None and not t.is_cuda:
        raise RuntimeError("position_induced_transformer_amd: the PiT hot path runs on the HIP device only; "
                           "got a CPU tensor (move the model and its inputs to 'cuda')")
    if t is not None and t.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"position_induced_transformer_amd: fp32 (or bf16-stored) tensor expected, got {t.dtype}")


def _need_gpu(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("position_induced_transformer_amd: the PiT hot path runs on the HIP device only; "
                               "got a CPU tensor (move the model and its inputs to 'cuda')")
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"position_induced_transformer_amd: fp32 tensors expected, got {t.dtype}")


def quantile_rank(locality: float, n_in: int):
    """(k, w) of torch.quantile's linear interpolation in ATen's fp32 arithmetic
    (SURVEY appendix A.3): rank = fl32(q)*fl32(n-1), k = floor(rank), w = rank - k."""
    rank = np.float32(locality) * np.float32(n_in - 1)
    k = int(np.floor(rank))
    w = np.float32(rank - np.float32(k))
    return k, float(w)


def mesh_period(metric: str, mesh_in: torch.Tensor) -> float:
    """Period of the periodic metrics, evaluated with the reference's own torch ops
    (pit.py:190-191 / 248-250).  One host sync; callers cache it per mesh."""
    if metric == "periodic1d":
        return float(torch.abs(mesh_in[1, 0] - mesh_in[0, 0]) * mesh_in.shape[0])
    if metric == "periodic2d":
        res = int(mesh_in.shape[0] ** 0.5)
        dx = (torch.max(mesh_in[:, 0]) - torch.min(mesh_in[:, 0])) / (res - 1)
        return float(dx * res)
    return 0.0


FOLD_SLAB_ROWS = (256, 128, 64)                              # slab heights MeshPlan.fold_plan tries, tallest first
# The fused decoder's slabs as 4 x 4 patches of a row-major output grid instead of 16 consecutive rows (pit_hip.h: pit_slab_plan,
# patch geometry): the rows of a patch list neighbouring keys, so a slab's key union - what its gather, tile copies and atomic adds scale
# with - is about half a strip's.  PIT_PATCH_SLABS=0: consecutive slabs everywhere (the A/B switch).
PATCH_SLABS = os.environ.get("PIT_PATCH_SLABS", "1") != "0"
PATCH_W = PATCH_H = 4


def row_major_grid(mesh: torch.Tensor):
    """(grid_w, grid_h) when ``mesh`` (n, 2) is EXACTLY a row-major tensor-product grid in the point order of
    np.meshgrid(xs, ys) flattened (tasks.grid_mesh_2d; coordinate 0 runs fastest): mesh[i*grid_w + j] == (xs[j], ys[i]) bit for bit,
    xs and ys strictly monotonic, both at least 4 long - index patches are then patches in space.  None for anything else: a
    column-major (transposed) grid, a perturbed or unstructured mesh, a 1-D mesh.  One small device-to-host copy: call it where a
    plan is built, never under stream capture."""
    if not torch.is_tensor(mesh) or mesh.dim() != 2 or mesh.shape[1] != 2 or mesh.shape[0] < 16 or not mesh.dtype.is_floating_point:
        return None
    m = mesh.detach().cpu()
    n = m.shape[0]
    moved = (m[:, 1] != m[0, 1]).nonzero()
    if moved.numel() == 0:
        return None
    gw = int(moved[0])
    if gw < 4 or n % gw or n // gw < 4:
        return None
    gh = n // gw
    g = m.view(gh, gw, 2)
    xs, ys = g[0, :, 0], g[:, 0, 1]
    if not (bool((g[:, :, 0] == xs[None, :]).all()) and bool((g[:, :, 1] == ys[:, None]).all())):
        return None
    mono = lambda v: bool((v[1:] > v[:-1]).all()) or bool((v[1:] < v[:-1]).all())
    return (gw, gh) if mono(xs) and mono(ys) else None
PLAN_FLAGS = 0                                               # pit_plan_fwd's `flags` (tests: 1 = PIT_PLAN_WAVE_PER_ROW, 2 = PIT_PLAN_TWO_PASSES)
UNION_TILES = os.environ.get("PIT_UNION_TILES", "auto")      # "auto" (probe per kind of plan), "0", "1"
UNION_DV = os.environ.get("PIT_UNION_DV", "auto")            # d(values) of union-tile layers: "auto", "lists" (transposed lists)
_UNION_DECISIONS = {}


def as_lengths(lengths, device, batch: int) -> torch.Tensor:
    """Per-sample point counts of a ragged batch as the kernels read them: a contiguous int32 tensor of shape (batch,) on
    ``device``.  A device tensor is used as it is when it already has that form (so a captured graph sees later in-place
    updates); int64 tensors and Python sequences are converted once.  Precondition, not checked (a check would synchronise):
    1 <= lengths[s] <= padded width - the kernels clamp into that range."""
    if torch.is_tensor(lengths):
        if lengths.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"lengths must be an int32 or int64 tensor, got {lengths.dtype}")
        t = lengths.detach().reshape(-1)
        if t.dtype != torch.int32 or t.device != device or not t.is_contiguous():
            t = t.to(device=device, dtype=torch.int32).contiguous()
    else:
        t = torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=device)
    if t.numel() != batch:
        raise ValueError(f"lengths must hold one entry per sample: {t.numel()} entries for a batch of {batch}")
    return t


RAGGED_LIST_CAP = None      # tests: force the list capacity of ragged plans (a small value makes rows overflow)


def ragged_list_capacity(rank_k: int, n_in: int) -> int:
    """Capacity of a ragged plan's candidate lists, from the PADDED width (so it does not depend on the lengths): k + 2 keys plus
    room for ties, as for any masked layer; 0 = no lists (not much shorter than the row, or beyond pit_lists_transpose's 4096 keys)."""
    if RAGGED_LIST_CAP is not None:
        return int(RAGGED_LIST_CAP)
    want = rank_k + 2
    cap = ((want + max(16, want // 4) + 15) // 16) * 16
    return 0 if (cap * 3 > n_in or n_in > 4096) else cap


def check_ragged(metric: str, mesh_out, mesh_in) -> None:
    """What a ragged batch (per-sample lengths) does not cover, refused before anything is launched."""
    if metric != "euclid":
        raise ValueError(f"lengths are defined for per-sample Euclidean meshes only, not for the {metric} metric")
    if mesh_out.dim() != 3 or mesh_in.dim() != 3:
        raise ValueError("lengths need per-sample (batch, n, space_dim) meshes: a batch-free mesh has no per-sample length")
    if mesh_grad_wanted(mesh_out, mesh_in):
        raise NotImplementedError("lengths with a mesh that requires grad: mesh gradients are not implemented for ragged batches")
    if get_math_mode() != "fp32":
        raise NotImplementedError("lengths in the bf16 math mode: ragged batches run in the fp32 math mode only")
    if mesh_out.shape[-1] > 3:
        raise NotImplementedError(f"lengths with space_dim > 3 (got {mesh_out.shape[-1]}): ragged batches take 1 to 3 coordinates")


def mixed_pair(mesh_out, mesh_in):
    """"out" / "in": which of the two meshes is the (n, space_dim) mesh SHARED by the whole batch when the other one is a
    (batch, n', space_dim) stack of per-sample clouds (the broadcast of pit.py:47-48); None for two meshes of one rank."""
    if not (torch.is_tensor(mesh_out) and torch.is_tensor(mesh_in)):
        return None
    if mesh_out.dim() == 2 and mesh_in.dim() == 3:
        return "out"
    if mesh_out.dim() == 3 and mesh_in.dim() == 2:
        return "in"
    return None


def check_mixed(metric: str, mesh_out, mesh_in, len_out=None, len_in=None) -> str:
    """What a shared mesh against per-sample clouds does not cover, refused before anything is launched; returns the shared side."""
    shared = mixed_pair(mesh_out, mesh_in)
    if (len_out if shared == "out" else len_in) is not None:
        raise ValueError("a length for the mesh shared by the batch: every one of its points is real for every sample - lengths "
                         "belong to the per-sample side only")
    if metric != "euclid":
        if len_out is not None or len_in is not None:
            raise ValueError(f"lengths are defined for per-sample Euclidean meshes only, not for the {metric} metric")
        raise RuntimeError("periodic metrics are defined for batch-free meshes only (pit.py:186-258)")
    if mesh_grad_wanted(mesh_out, mesh_in):
        raise NotImplementedError("a mesh that requires grad in a mixed pair: mesh gradients are not implemented for a shared mesh "
                                  "against per-sample clouds")
    if len_out is not None or len_in is not None:
        if get_math_mode() != "fp32":
            raise NotImplementedError("lengths in the bf16 math mode: ragged batches run in the fp32 math mode only")
        if mesh_out.shape[-1] > 3:
            raise NotImplementedError(f"lengths with space_dim > 3 (got {mesh_out.shape[-1]}): ragged batches take 1 to 3 coordinates")
    return shared


class MeshPlan:
    """Everything about a (mesh_out, mesh_in, metric, locality) pair that does not depend on
    lmda: contiguous 3-d meshes, period, quantile rank and the selection statistics
    (m_(k), m_(k+1), m_min per row).  Fixed meshes build it once and reuse it every step."""

    __slots__ = ("mesh_out", "mesh_in", "mesh_batch", "n_out", "n_in", "sdim", "metric", "metric_id", "period",
                 "rank_k", "rank_w", "masked", "self_attn", "stats", "nbr_idx", "nbr_cnt", "nbr_cap", "rev_ptr",
                 "rev_row", "_complete", "_union", "_slab", "_patch", "_fold", "len_out", "len_in", "rank_w_dev", "shared", "_rev_sorted")

    def __init__(self, metric: str, mesh_out: torch.Tensor, mesh_in: torch.Tensor, locality: float,
                 self_attn: bool, period: Optional[float] = None, len_out=None, len_in=None):
        """``len_out`` / ``len_in`` (both or neither; self attention: the same object): per-sample point counts of a ragged
        batch (``as_lengths``).  The plan then holds the statistics of pit_plan_ragged_fwd - rank and interpolation weight are
        formed per sample on the device - and its layers run on the pit_posatt_ragged_* entries only.
        A MIXED pair - one (n, s) mesh shared by the batch, one (b, n', s) stack of clouds - means "the same n points for every
        sample" (``shared`` = "out" / "in").  Only the cloud side can have a length; with one the plan keeps the shared mesh as it
        is (a detached contiguous view, as for batch-free meshes: no copy) and its layers run on the pit_posatt_ragged_strided_*
        entries, which read it in place; without one the plan holds an expanded (b, n, s) copy of the shared mesh, made once here,
        and is from then on a per-sample plan like any other: the default kernels, untouched."""
        self.len_out = self.len_in = self.rank_w_dev = None
        self.shared = mixed_pair(mesh_out, mesh_in)
        if self.shared is not None:
            if metric not in METRIC_ID:
                raise ValueError(f"unknown metric {metric!r}")
            check_mixed(metric, mesh_out, mesh_in, len_out, len_in)
            _need_gpu(mesh_out, mesh_in)
            if mesh_out.shape[-1] != mesh_in.shape[-1]:
                raise RuntimeError("mesh_out and mesh_in must have the same number of coordinates")
            if len_out is None and len_in is None:
                b = (mesh_in if self.shared == "out" else mesh_out).shape[0]
                if self.shared == "out":
                    mesh_out = mesh_out.detach().unsqueeze(0).expand(b, -1, -1).contiguous()
                else:
                    mesh_in = mesh_in.detach().unsqueeze(0).expand(b, -1, -1).contiguous()
        elif len_out is not None or len_in is not None:
            if len_out is None or len_in is None:
                raise ValueError("a ragged plan needs both len_out and len_in")
            if metric not in METRIC_ID:
                raise ValueError(f"unknown metric {metric!r}")
            check_ragged(metric, mesh_out, mesh_in)
        _need_gpu(mesh_out, mesh_in)
        if metric not in METRIC_ID:
            raise ValueError(f"unknown metric {metric!r}")
        ragged_mixed = self.shared is not None and (len_out is not None or len_in is not None)
        if (mesh_out.dim() != mesh_in.dim() and not ragged_mixed) or mesh_out.dim() not in (2, 3) or mesh_in.dim() not in (2, 3):
            raise RuntimeError(f"mesh shapes {tuple(mesh_out.shape)} / {tuple(mesh_in.shape)} not supported")
        if mesh_out.shape[-1] != mesh_in.shape[-1]:
            raise RuntimeError("mesh_out and mesh_in must have the same number of coordinates")
        batched = mesh_out.dim() == 3 or mesh_in.dim() == 3
        if batched and metric != "euclid":
            raise RuntimeError("periodic metrics are defined for batch-free meshes only (pit.py:186-258)")
        if batched and not ragged_mixed and mesh_out.shape[0] != mesh_in.shape[0]:
            raise RuntimeError("batched meshes must share the batch size")
        self.metric = metric
        self.metric_id = METRIC_ID[metric]
        self.mesh_out = mesh_out.detach().contiguous()
        self.mesh_in = self.mesh_out if (self_attn and mesh_in is mesh_out) else mesh_in.detach().contiguous()
        self.mesh_batch = (mesh_out if mesh_out.dim() == 3 else mesh_in).shape[0] if batched else 1
        self.n_out, self.n_in, self.sdim = mesh_out.shape[-2], mesh_in.shape[-2], mesh_out.shape[-1]
        if not 1 <= self.sdim <= MAX_SPACE_DIM:
            raise RuntimeError(f"space_dim must be between 1 and {MAX_SPACE_DIM}, got {self.sdim}")
        self.period = mesh_period(metric, self.mesh_in) if period is None else float(period)
        self.rank_k, self.rank_w = quantile_rank(locality, self.n_in)
        self.masked = bool(locality < 1.0)
        self.self_attn = bool(self_attn)
        self.stats = None
        self.nbr_idx = self.nbr_cnt = self.rev_ptr = self.rev_row = None
        self.nbr_cap = 0
        self._complete = None
        self._rev_sorted = None
        self._union = None
        self._slab = None
        self._patch = None
        self._fold = None
        if ragged_mixed:
            # a shared mesh against ragged clouds: the plan of a ragged batch below, on the strided entries - stride 0 and no
            # length on the shared side.  The list capacity comes from the full (shared keys) or padded (cloud keys) width, as
            # ragged_list_capacity chooses it for the expanded pair; lists and their transpose are per sample either way
            dev, mb = mesh_out.device, self.mesh_batch
            self.len_out = None if len_out is None else as_lengths(len_out, dev, mb)
            self.len_in = None if len_in is None else as_lengths(len_in, dev, mb)
            self.stats = torch.empty((3, mb, self.n_out), device=dev, dtype=torch.float32)
            self.rank_w_dev = torch.empty((mb,), device=dev, dtype=torch.float32)
            cap = ragged_list_capacity(self.rank_k, self.n_in) if (self.masked and SPARSE_MASKED) else 0
            if cap:
                self.nbr_cap = cap
                self.nbr_idx = torch.empty((mb, self.n_out, cap), device=dev, dtype=torch.int32)
                self.nbr_cnt = torch.empty((mb, self.n_out), device=dev, dtype=torch.int32)
            so, si = self.sample_strides()
            rc = _lib.lib().pit_plan_ragged_strided_fwd(self.mesh_out.data_ptr(), self.mesh_in.data_ptr(), mb, self.n_out,
                                                        self.n_in, self.sdim, so, si, _lib.ptr(self.len_out), _lib.ptr(self.len_in),
                                                        float(np.float32(locality)), 1 if self.masked else 0, self.stats.data_ptr(),
                                                        self.rank_w_dev.data_ptr(), cap, _lib.ptr(self.nbr_idx),
                                                        _lib.ptr(self.nbr_cnt), _lib.stream_ptr())
            _lib.check(rc, "pit_plan_ragged_strided_fwd")
            if cap and torch.is_grad_enabled():          # the transposed lists, per sample: d(values) is per sample
                self.rev_ptr = torch.empty((mb, self.n_in + 1), device=dev, dtype=torch.int32)
                self.rev_row = torch.empty((mb, self.n_out * cap), device=dev, dtype=torch.int32)
                ws = torch.empty((2 * mb * self.n_in,), device=dev, dtype=torch.int32)
                rc = _lib.lib().pit_lists_transpose(self.nbr_idx.data_ptr(), self.nbr_cnt.data_ptr(), mb, self.n_out, self.n_in, cap,
                                                    self.rev_ptr.data_ptr(), self.rev_row.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
                _lib.check(rc, "pit_lists_transpose")
            if _capturing():
                _pin(self.len_out, self.len_in, self.mesh_out, self.mesh_in)
            return
        if len_out is not None:
            # ragged batch: statistics over the first len_in[s] keys, rank and weight per sample on the device (rank_k / rank_w
            # above are those of the padded width: they only size the lists).  Candidate lists as for any masked layer: the
            # capacity comes from the PADDED width, so it does not depend on the lengths; overflowed rows scan all keys
            self.len_out = as_lengths(len_out, mesh_out.device, self.mesh_batch)
            self.len_in = self.len_out if len_in is len_out else as_lengths(len_in, mesh_out.device, self.mesh_batch)
            dev, mb = mesh_out.device, self.mesh_batch
            self.stats = torch.empty((3, mb, self.n_out), device=dev, dtype=torch.float32)
            self.rank_w_dev = torch.empty((mb,), device=dev, dtype=torch.float32)
            cap = ragged_list_capacity(self.rank_k, self.n_in) if (self.masked and SPARSE_MASKED) else 0
            if cap:
                self.nbr_cap = cap
                self.nbr_idx = torch.empty((mb, self.n_out, cap), device=dev, dtype=torch.int32)
                self.nbr_cnt = torch.empty((mb, self.n_out), device=dev, dtype=torch.int32)
            rc = _lib.lib().pit_plan_ragged_fwd(self.mesh_out.data_ptr(), self.mesh_in.data_ptr(), mb, self.n_out,
                                                self.n_in, self.sdim, self.len_out.data_ptr(), self.len_in.data_ptr(),
                                                float(np.float32(locality)), 1 if self.masked else 0, self.stats.data_ptr(),
                                                self.rank_w_dev.data_ptr(), cap, _lib.ptr(self.nbr_idx), _lib.ptr(self.nbr_cnt),
                                                _lib.stream_ptr())
            _lib.check(rc, "pit_plan_ragged_fwd")
            if cap and torch.is_grad_enabled():          # the transposed lists: d(values) walks them by key
                self.rev_ptr = torch.empty((mb, self.n_in + 1), device=dev, dtype=torch.int32)
                self.rev_row = torch.empty((mb, self.n_out * cap), device=dev, dtype=torch.int32)
                ws = torch.empty((2 * mb * self.n_in,), device=dev, dtype=torch.int32)
                rc = _lib.lib().pit_lists_transpose(self.nbr_idx.data_ptr(), self.nbr_cnt.data_ptr(), mb, self.n_out, self.n_in, cap,
                                                    self.rev_ptr.data_ptr(), self.rev_row.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
                _lib.check(rc, "pit_lists_transpose")
            if _capturing():
                _pin(self.len_out, self.len_in)
            return
        cap = 0
        if self.masked and SPARSE_MASKED:
            want = self.rank_k + 2
            cap = ((want + max(16, want // 4) + 15) // 16) * 16        # k+2 keys plus room for ties
            if cap * 3 > self.n_in:
                cap = 0                                                 # lists not much shorter than the row: dense
        if self.masked or not self.self_attn:
            self.stats = torch.empty((3, self.mesh_batch, self.n_out), device=mesh_out.device, dtype=torch.float32)
        if cap:
            self._build_lists(cap, self._wants_reverse_lists(cap))      # selection + lists in one pass
        elif self.stats is not None:
            name = "pit_select_fwd" if self.sdim <= 3 else "pit_select_wide_fwd"     # (the first keeps space_dim 1..3)
            rc = getattr(_lib.lib(), name)(self.mesh_out.data_ptr(), self.mesh_in.data_ptr(), self.mesh_batch,
                                           self.n_out, self.n_in, self.sdim, self.metric_id, self.period,
                                           self.rank_k, 1 if self.masked else 0, self.stats.data_ptr(),
                                           _lib.stream_ptr())
            _lib.check(rc, name)

    def ragged(self) -> bool:
        """The plan of a ragged batch: its layers run on the pit_posatt_ragged_* entries."""
        return self.len_out is not None or self.len_in is not None

    def sample_strides(self):
        """(out, in) sample strides in points for the strided ragged entries: 0 for the mesh shared by the batch."""
        return (0 if self.mesh_out.dim() == 2 else self.n_out, 0 if self.mesh_in.dim() == 2 else self.n_in)

    def _union_key(self, cap):
        return (self.metric, self.n_out, self.n_in, cap, self.mesh_batch > 1, self.sdim)

    def _wants_reverse_lists(self, cap: int) -> bool:
        """The transposed lists (key -> rows) serve d(values) of the candidate-list kernels only.  Plans of meshes shared by the
        batch are cached: built once, with them.  Per-sample plans are rebuilt EVERY step (train_naca.py:62-65): built without,
        and the backward that needs them (d(values) requested and not supplied by the union tiles) builds them on demand
        (ensure_reverse_lists) - an encoder whose inputs need no gradient never pays for them (NACA: 33 us, Elasticity 45 us per
        step), nor does a union-tile layer (NACA decoder: 93 us)."""
        return self.mesh_batch == 1

    def ensure_reverse_lists(self) -> None:
        if self.nbr_idx is None or self.rev_ptr is not None:
            return
        dev = self.mesh_out.device
        rev_ptr = torch.empty((self.mesh_batch, self.n_in + 1), device=dev, dtype=torch.int32)
        rev_row = torch.empty((self.mesh_batch, self.n_out * self.nbr_cap), device=dev, dtype=torch.int32)
        work = torch.empty((2 * self.mesh_batch * self.n_in,), device=dev, dtype=torch.int32)
        rc = _lib.lib().pit_lists_transpose(self.nbr_idx.data_ptr(), self.nbr_cnt.data_ptr(), self.mesh_batch, self.n_out,
                                            self.n_in, self.nbr_cap, rev_ptr.data_ptr(), rev_row.data_ptr(), work.data_ptr(),
                                            _lib.stream_ptr())
        if rc == _ERR_UNSUPPORTED:                      # (rows longer than 4096 keys): the whole plan again
            self._build_lists(self.nbr_cap, True)
            return
        _lib.check(rc, "pit_lists_transpose")
        self.rev_ptr, self.rev_row = rev_ptr, rev_row

    def sorted_reverse_lists(self) -> torch.Tensor:
        """The transposed lists with every key's range in ascending row order, -1 slots (overflowed rows) last
        (pit_lists_sort_ranges): pit_lists_transpose fills a range in whatever order its atomics land, and d(values) is summed
        in list order.  The reproducible mode reads this copy; ``rev_row`` itself stays as it was built, so a plan that was
        cached with the mode off serves both (``_rev_sorted`` is the flag: built on first use in the mode)."""
        if self._rev_sorted is None or self._rev_sorted[0] is not self.rev_row:
            out = self.rev_row.clone()                  # (slots outside every range keep their contents)
            rc = _lib.lib().pit_lists_sort_ranges(self.rev_ptr.data_ptr(), self.rev_row.data_ptr(), self.mesh_batch, self.n_in,
                                                  self.n_out * self.nbr_cap, out.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "pit_lists_sort_ranges")
            self._rev_sorted = (self.rev_row, out)
        return self._rev_sorted[1]

    def union_tiles(self) -> bool:
        """Round 4: do the masked-layer kernels take the UNION-TILE form (PIT_ATT_UNION) for this plan?  They contract 16
        consecutive rows against the union of their candidate keys: fast when neighbouring rows share their keys (grids,
        body-fitted meshes), slow for incoherent orderings (random clouds) - never wrong.  Decided ONCE per kind of plan
        (metric, sizes, capacity, batched or not) from 32 sampled tiles of the first plan of that kind built outside a
        stream capture (the probe synchronises); plans built under capture before any probe keep the per-row kernels."""
        if self._union is not None:
            return self._union
        # (meshes shared by the batch: the per-row kernels already stream batch x dim wide rows at the HBM rate - measured)
        if self.nbr_idx is None or UNION_TILES == "0" or self.n_in > 4096 or self.n_out < 16 or self.nbr_cap > 64 \
                or (self.mesh_batch == 1 and UNION_TILES != "1"):
            self._union = False
            return False
        if UNION_TILES == "1":
            self._union = True
            return True
        key = self._union_key(self.nbr_cap)
        hit = _UNION_DECISIONS.get(key)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                return False                             # (not cached: a later eager plan of this kind may still probe)
            # 32 tiles of 16 consecutive rows of the first sample: sizes of the unions of their candidate lists
            cap, tiles = self.nbr_cap, min(32, self.n_out // 16)
            first = (torch.linspace(0, self.n_out // 16 - 1, tiles).long() * 16).to(self.nbr_idx.device)
            rows = (first[:, None] + torch.arange(16, device=first.device)[None, :]).reshape(-1)
            idx = self.nbr_idx.view(-1, cap)[rows].long()
            cnt = self.nbr_cnt[rows].long()
            keys = torch.where(torch.arange(cap, device=first.device)[None, :] < cnt[:, None], idx, -1).view(tiles, 16 * cap)
            srt = torch.sort(keys, dim=1).values
            union = (srt[:, 1:] != srt[:, :-1]).sum(1) + 1 - (srt[:, 0] < 0).long()
            mean_u, mean_k, over = (float(v) for v in torch.stack(
                [union.float().mean(), cnt.float().mean(), (cnt > cap).float().max()]).tolist())
            # MFMA work ~ union size, the per-row kernels' ~ list length; one chunk of the kernel holds 64 union keys
            hit = over == 0.0 and mean_u <= min(64.0, 4.0 * mean_k)
            _UNION_DECISIONS[key] = hit
        self._union = hit
        return hit

    def slab_plan(self, patch: bool = False):
        """Round 5: the static per-slab plan of this (fixed) mesh pair for the fused encoder- / decoder-side launches
        (csrc/pit_edge.hip; include/pit_hip.h: pit_slab_plan) as (struct, largest union of a 16-row slab's candidate keys), or
        None: per-sample meshes, no candidate lists, a list that overflowed its capacity.  Built once per plan - the meshes are
        batch-free and cached - with one host read of two ints; never under stream capture (a plan first seen there keeps the
        per-layer kernels).  ``patch`` (the fused decoder only): the plan whose slabs are 4 x 4 patches of the output grid when
        mesh_out is a row-major grid (row_major_grid), cached next to the consecutive one; the consecutive plan otherwise."""
        # (a plan first asked for a patch plan under stream capture - building one reads the mesh on the host - runs on its
        # consecutive plan, if that one is cached, like any plan that has no patch plan)
        if patch and PATCH_SLABS and self._patch is not False and not (self._patch is None and torch.cuda.is_current_stream_capturing()):
            if self._patch is None:
                self._patch = False
                eligible = not (self.nbr_idx is None or self.mesh_batch != 1 or not self.masked or self.n_in > 16384 or self.nbr_cap > 64)
                grid = row_major_grid(self.mesh_out) if eligible else None
                if grid is not None:
                    built = self._build_slab_plan(16, grid + (PATCH_W, PATCH_H))
                    if built is not None and built[1] <= SLAB_UNION_MAX:
                        self._patch = built
            if self._patch:
                return self._patch
        if self._slab is not None:
            return self._slab or None
        if self.nbr_idx is None or self.mesh_batch != 1 or not self.masked or self.n_in > 16384 or self.nbr_cap > 64:
            self._slab = False
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        dev = self.mesh_out.device
        built = self._build_slab_plan(16)
        if built is None:
            self._slab = False
            return None
        self._slab = built
        return self._slab

    def _build_slab_plan(self, rows: int, geo=None):
        """pit_slab_plan_build for slabs of `rows` rows: (struct, largest union, keep-alive tensors, longest list) or None when a
        candidate list overflowed its capacity (one host read of three ints).  ``geo`` = (grid_w, grid_h, patch_w, patch_h):
        pit_slab_plan_build_patch, the slabs are patches of the row-major output grid."""
        dev = self.mesh_out.device
        if geo is not None:
            gw, gh, pw, ph = geo
            n_slabs = -(-gh // ph) * -(-gw // pw)
        else:
            n_slabs = (self.n_out + rows - 1) // rows
        m = torch.empty((n_slabs * rows, self.nbr_cap), device=dev, dtype=torch.float32)
        slot = torch.empty((n_slabs * rows, self.nbr_cap), device=dev, dtype=torch.int16)
        keys = torch.empty((n_slabs, SLAB_UNION_MAX), device=dev, dtype=torch.int32)
        nkeys = torch.empty((n_slabs,), device=dev, dtype=torch.int32)
        report = torch.zeros((3,), device=dev, dtype=torch.int32)
        if geo is not None:
            rc = _lib.lib().pit_slab_plan_build_patch(self.mesh_out.data_ptr(), self.mesh_in.data_ptr(), self.n_out, self.n_in,
                                                      self.sdim, self.metric_id, self.period, self.nbr_idx.data_ptr(),
                                                      self.nbr_cnt.data_ptr(), self.nbr_cap, gw, gh, pw, ph, self.stats.data_ptr(),
                                                      self.rank_w, m.data_ptr(), slot.data_ptr(), keys.data_ptr(),
                                                      nkeys.data_ptr(), report.data_ptr(), _lib.stream_ptr())
        else:
            rc = _lib.lib().pit_slab_plan_build(self.mesh_out.data_ptr(), self.mesh_in.data_ptr(), self.n_out, self.n_in, self.sdim,
                                                self.metric_id, self.period, self.nbr_idx.data_ptr(), self.nbr_cnt.data_ptr(),
                                                self.nbr_cap, rows, m.data_ptr(), slot.data_ptr(), keys.data_ptr(), nkeys.data_ptr(),
                                                report.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_slab_plan_build")
        max_union, overflowed, max_count = report.tolist()
        if overflowed:
            return None
        sp = _lib.SlabPlan(self.n_out, self.n_in, self.nbr_cap, n_slabs, SLAB_UNION_MAX, self.stats.data_ptr(), self.rank_w,
                           self.nbr_idx.data_ptr(), self.nbr_cnt.data_ptr(), m.data_ptr(), slot.data_ptr(), keys.data_ptr(),
                           nkeys.data_ptr(), rows, *(geo or (0, 0, 0, 0)))
        return (sp, int(max_union), (m, slot, keys, nkeys), max(1, int(max_count)))

    def fold_plan(self):
        """Round 6: the slab plan of the folded decoder (csrc/pit_fold.hip) - the TALLEST slabs (256, 128, 64 rows) whose candidate
        keys' union still fits a tile (64 keys): the taller, the fewer adds d(values) costs.  None: per-sample meshes, no lists,
        an overflowed list, or unions beyond 64 keys even at 64 rows (incoherently ordered meshes).  Built once, never under
        stream capture."""
        if self._fold is not None:
            return self._fold or None
        if self.nbr_idx is None or self.mesh_batch != 1 or not self.masked or self.n_in > 16384 or self.nbr_cap > 64 \
                or self.n_out < 64:
            self._fold = False
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        for rows in FOLD_SLAB_ROWS:
            built = self._build_slab_plan(rows)
            if built is None:
                break
            if built[1] <= SLAB_UNION_MAX:
                # key -> the (slab, slot) entries that hold it (CSR, in slab order): the backward's tiles are summed per key in this
                # fixed order instead of being added to memory with atomics
                sp, mu, keep, mc = built
                keys, nkeys = keep[2], keep[3]
                n_slabs = keys.shape[0]
                slot = torch.arange(SLAB_UNION_MAX, device=keys.device, dtype=torch.int64)[None, :].expand(n_slabs, -1)
                valid = slot < nkeys[:, None].long()
                ent = (torch.arange(n_slabs, device=keys.device, dtype=torch.int64)[:, None] * SLAB_UNION_MAX + slot)[valid]
                key = keys.long()[valid]
                order = torch.sort(key, stable=True).indices
                rev_ent = ent[order].to(torch.int32).contiguous()
                rev_ptr = torch.zeros((self.n_in + 1,), device=keys.device, dtype=torch.int64)
                rev_ptr[1:] = torch.cumsum(torch.bincount(key, minlength=self.n_in), 0)
                rev_ptr = rev_ptr.to(torch.int32).contiguous()
                self._fold = (sp, mu, keep + (rev_ptr, rev_ent), mc)
                return self._fold
        self._fold = False
        return None

    def lists_complete(self) -> int:
        """1 if no row's candidate list overflowed its capacity (checked once, for batch-free meshes
        whose plan is cached; never during stream capture - the check synchronises), else 0."""
        if self.nbr_cnt is None or self.mesh_batch != 1:
            return 0
        if self._complete is None:
            if torch.cuda.is_current_stream_capturing():
                return 0
            self._complete = int(bool((self.nbr_cnt <= self.nbr_cap).all().item()))
        return self._complete

    def _build_lists(self, cap: int, reverse: bool = True) -> None:
        """Order statistics, candidate lists (row -> keys) and - with `reverse` - their transpose (key -> rows) for the
        sparse kernels, one pass over the rows (pit_plan_fwd)."""
        dev = self.mesh_out.device
        rows = self.mesh_batch * self.n_out
        L = _lib.lib()
        self.nbr_cap = cap
        self.nbr_idx = torch.empty((rows, cap), device=dev, dtype=torch.int32)
        self.nbr_cnt = torch.empty((rows,), device=dev, dtype=torch.int32)
        work = None
        if reverse:
            self.rev_ptr = torch.empty((self.mesh_batch, self.n_in + 1), device=dev, dtype=torch.int32)
            self.rev_row = torch.empty((self.mesh_batch, self.n_out * cap), device=dev, dtype=torch.int32)
            work = torch.empty((2 * self.mesh_batch * self.n_in,), device=dev, dtype=torch.int32)
        rc = L.pit_plan_fwd(self.mesh_out.data_ptr(), self.mesh_in.data_ptr(), self.mesh_batch, self.n_out,
                            self.n_in, self.sdim, self.metric_id, self.period, self.rank_k, self.stats.data_ptr(), cap,
                            self.nbr_idx.data_ptr(), self.nbr_cnt.data_ptr(), _lib.ptr(self.rev_ptr),
                            _lib.ptr(self.rev_row), _lib.ptr(work), int(PLAN_FLAGS), _lib.stream_ptr())
        _lib.check(rc, "pit_plan_fwd")


def _row_view(t: torch.Tensor) -> torch.Tensor:
    """(b, L, D) tensor with unit channel stride (copy only if it is not already so)."""
    if t.dim() != 3:
        raise RuntimeError(f"expected a (batch, points, channels) tensor, got {tuple(t.shape)}")
    if t.stride(2) != 1 or t.stride(1) < t.shape[2]:
        t = t.contiguous()
    return t


UNION_ATT = os.environ.get("PIT_UNION_ATT", "1") != "0"
# bf16 mode: dense self-attention of hid 128 / 256 on csrc/pit_satt.hip.  "auto": where it measured faster than the fp32-era kernels
# with rounded operands - layers of >= 256 points (per layer, with the weight tiles and the operands written by the neighbouring MLP
# chains: Elasticity 972 x 256 x 2 heads ~105 us against 191, NACA 728 x 128 x 1 ~55 against 70, Vorticity 256 x 256 x 2 ~36 against
# 47 - DESIGN.md section 4 round 6; shorter layers: not measured); "1": every supported shape; "0": never
SATT = os.environ.get("PIT_SATT", "auto")
SATT_TILES = os.environ.get("PIT_SATT_TILES", "1") != "0"      # the forward keeps its weights as bf16 tiles for the backward
SATT_FUSE_PREP = os.environ.get("PIT_SATT_FUSE_PREP", "1") != "0"      # the MLP chains either side write the bf16 operands (no prep launches)
SATT_DW_RIDER = os.environ.get("PIT_SATT_DW_RIDER", "1") != "0"        # the consuming MLP's dW / db reductions ride in the layer's backward launch
WIDE_DW_RIDER = os.environ.get("PIT_WIDE_DW_RIDER", "1") != "0"        # the same for dense layers on posatt_bwd_pair_wide_kernel (fp32 mode, large regime)


def _satt_pays(n_pts: int, n_head: int, d: int) -> bool:
    if SATT == "auto":
        return n_pts >= 256
    return SATT not in ("0", "", False)


# The hand-offs are checked by address AND version counter: an in-place edit of the values between the producing chain and the
# attention, or a gradient accumulated into / scaled in the consuming chain's d_x buffer by autograd or a hook, keeps the address but
# leaves the bf16 copy stale - the prep launch then forms it again from what the tensor holds now.
def _handoff_x16(values: torch.Tensor):
    """bf16(values) written by the producing MLP chain (mlp_apply), or None if there is none or ``values`` changed since."""
    x16 = getattr(values, "_pit_x16", None)
    if x16 is None or getattr(values, "_pit_x16_version", None) != values._version:
        return None
    return x16


def _handoff_g16_ready(link, d_out: torch.Tensor, shape) -> bool:
    """True if the consuming chain's G16 (link["g16"]) was formed from exactly this d_out: its buffer, unchanged since."""
    g16 = link.get("g16") if link is not None else None
    return (g16 is not None and link.get("dx_ptr") == d_out.data_ptr() and link.get("dx_version") == d_out._version
            and tuple(g16.shape) == tuple(shape))


def _union_att_ok(plan: "MeshPlan", n_head: int, d: int, b: int, values: torch.Tensor) -> bool:
    if torch.are_deterministic_algorithms_enabled():       # (d(values) leaves these kernels as fp32 atomic adds)
        return False
    if not (plan.mesh_batch == 1 and plan.masked and plan.nbr_idx is not None and not plan.self_attn and n_head in (1, 2)
            and d % 64 == 0 and d >= UNION_ATT_MIN_DIM and plan.sdim <= 3):
        return False
    if values.stride(1) % 4 or values.stride(0) % 4 or values.data_ptr() % 16:
        return False
    if not _lib.lib().pit_union_att_supported(int(n_head), int(d), int(b), int(plan.n_out)):
        return False
    sp = plan.slab_plan()
    return sp is not None and sp[1] <= SLAB_UNION_MAX


UNION_ATT_MIN_DIM = 128            # (width 64 models take the fused decoder launch; a layer that cannot keeps the candidate-list kernels)


def mesh_grad_wanted(*meshes) -> bool:
    """True when autograd records and one of the mesh tensors requires grad: the forward then takes the per-layer path whose
    attention layers pass the meshes to _PosAtt (pit.py:47,134 differentiates through the coordinates)."""
    return torch.is_grad_enabled() and any(torch.is_tensor(m) and m.requires_grad for m in meshes)


def _check_mesh_grad(metric: str) -> None:
    """Refusals of the mesh-gradient path, raised before anything is launched."""
    if metric != "euclid":
        raise NotImplementedError(
            f"gradients w.r.t. the mesh coordinates are implemented for the Euclidean metric only, not {metric!r}: the reference "
            "also differentiates through the period and the minimum / abs tie rules of the periodic distances (pit.py:190-191,248-250)")
    if get_math_mode() != "fp32":
        raise NotImplementedError(
            "gradients w.r.t. the mesh coordinates are implemented for the fp32 math mode only (set_math_mode('fp32')): the bf16 "
            "mode's rounded weights are not the ones the closed-form mesh gradient re-forms")


def _mesh_grads(ctx, values, head, rowstat, scale, d_out):
    """(d mesh_out, d mesh_in) of a _PosAtt layer: pit_posatt_dmesh after the layer's d(values) / d(head) launches."""
    if not getattr(ctx, "mesh_grad", False):
        return None, None
    need_o, need_i = ctx.needs_input_grad[12], ctx.needs_input_grad[13]
    if ctx.mesh_same:
        need_o = need_i = need_o or need_i
    if not (need_o or need_i):
        return None, None
    plan, n_head = ctx.plan, ctx.n_head
    b, j, dv = values.shape
    if d_out.dtype != torch.float32:
        d_out = d_out.float()
    d_out = _row_view(d_out)
    dev = values.device
    d_mo = torch.empty(plan.mesh_out.shape, device=dev, dtype=torch.float32) if need_o else None
    d_mi = d_mo if ctx.mesh_same else (torch.empty(plan.mesh_in.shape, device=dev, dtype=torch.float32) if need_i else None)
    if need_i and plan.nbr_idx is not None:
        plan.ensure_reverse_lists()
    L = _lib.lib()
    ws = torch.empty(((L.pit_posatt_dmesh_workspace(plan.mesh_batch, plan.n_out, plan.n_in, plan.sdim, b, n_head) + 3) // 4,),
                     device=dev, dtype=torch.float32)
    rc = L.pit_posatt_dmesh(
        plan.mesh_out.data_ptr(), plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_out, plan.n_in, plan.sdim,
        plan.metric_id, plan.period,
        values.data_ptr(), b, dv, values.stride(1), values.stride(0),
        head.data_ptr(), n_head, 1 if ctx.head_is_scale else 0, scale.data_ptr(),
        rowstat.data_ptr(), 1 if plan.masked else 0,
        d_out.data_ptr(), d_out.stride(1), d_out.stride(0), dv if ctx.concat else 0,
        _lib.ptr(plan.nbr_idx), _lib.ptr(plan.nbr_cnt), plan.nbr_cap, plan.lists_complete(),
        _lib.ptr(plan.rev_ptr), _lib.ptr(plan.rev_row),
        _lib.ptr(d_mo), _lib.ptr(d_mi), 0, ws.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "pit_posatt_dmesh")
    if ctx.mesh_same:
        return d_mo.view(ctx.mesh_shapes[0]), None
    return (d_mo.view(ctx.mesh_shapes[0]) if d_mo is not None else None,
            d_mi.view(ctx.mesh_shapes[1]) if d_mi is not None else None)


def _layer_outputs(values, head, plan, n_head: int, concat: bool, refusals, shared_ok: bool):
    """What a layer node on a plan beside the main path does before its launch: checks (values, head, plan, n_head, concat) and
    allocates out, rowstat and scale.  ``refusals``: the plan's words for a wrong point count, a wrong batch and a concat whose
    two sides differ (None: not checked); ``shared_ok``: one geometry may serve the whole batch.  Returns the row view of the
    values and the flat head with them."""
    _need_gpu(values, head)
    values = _row_view(values)
    b, j, d = values.shape
    points, batch, square = refusals
    if j != plan.n_in:
        raise RuntimeError(points.format(j=j, n_in=plan.n_in))
    if plan.mesh_batch != b and not (shared_ok and plan.mesh_batch == 1):
        raise RuntimeError(batch)
    if square is not None and concat and plan.n_out != plan.n_in:
        raise RuntimeError(square)
    head = head.detach().reshape(-1).contiguous()
    if head.numel() != n_head:
        raise RuntimeError("lmda must hold one value per head")
    width = (n_head + (1 if concat else 0)) * d
    out = torch.empty((b, plan.n_out, width), device=values.device, dtype=torch.float32)
    rowstat = torch.empty((plan.mesh_batch, n_head, plan.n_out, 4), device=values.device, dtype=torch.float32)
    scale = torch.empty((n_head,), device=values.device, dtype=torch.float32)
    return values, head, out, rowstat, scale


def _layer_io(values, head, n_head: int, is_scale: bool, concat: bool, with_batch: bool, rowstat, scale, out=None,
              d_out=None, d_values=None, d_head=None, work=None):
    """The argument groups of a layer entry (_lib.values_args ...) around which a plan places its geometry and extras: of a
    forward entry when ``out`` is given, of a backward entry when ``d_out`` is."""
    b, j, d = values.shape
    io = types.SimpleNamespace(batch=b, dim=d, n_head=n_head, values=_lib.values_args(values, with_batch),
                               tail=(MATH_MODES["fp32"], _lib.stream_ptr()))
    if d_out is None:
        io.head = _lib.head_args(head, n_head, is_scale)
        io.out = _lib.out_args(out, d, concat, rowstat, scale)
    else:
        io.head = _lib.head_args(head, n_head, is_scale, scale)
        io.rowstat = rowstat.data_ptr()
        io.d_out = _lib.dout_args(d_out, d, concat)
        io.d_values = _lib.dvalues_args(d_values, j, d, concat)
        io.d_head = _lib.dhead_args(d_head, work)
    return io


class _PosAttRagged(torch.autograd.Function):
    """_PosAtt on a ragged plan (MeshPlan with lengths): pit_posatt_ragged_fwd / _bwd, one launch per layer and direction
    (+ the d(lmda) finish); none of the fused / union / tiled / paired launches is taken."""

    @staticmethod
    def _geometry(plan: MeshPlan, direction: str):
        # (a shared mesh against ragged clouds: the strided entries - stride 0, no length on the shared side)
        entry, extra = ("pit_posatt_ragged_", ()) if plan.shared is None else ("pit_posatt_ragged_strided_", plan.sample_strides())
        return entry + direction, (plan.mesh_out.data_ptr(), plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_out, plan.n_in, plan.sdim,
                                   *extra, _lib.ptr(plan.len_out), _lib.ptr(plan.len_in))

    @staticmethod
    def forward(ctx, values, head, plan: MeshPlan, n_head: int, concat: bool, head_is_scale: bool):
        refusals = ("inputs have {j} points but mesh_in has {n_in}", "mesh batch and input batch differ", None)
        values, head, out, rowstat, scale = _layer_outputs(values, head, plan, n_head, concat, refusals, False)
        io = _layer_io(values, head, n_head, head_is_scale, concat, False, rowstat, scale, out=out)
        entry, geometry = _PosAttRagged._geometry(plan, "fwd")
        rc = getattr(_lib.lib(), entry)(
            *geometry, *io.values, *io.head, plan.stats.data_ptr(), plan.rank_w_dev.data_ptr(), 1 if plan.masked else 0, *io.out,
            _lib.ptr(plan.nbr_idx), _lib.ptr(plan.nbr_cnt), plan.nbr_cap, *io.tail)
        _lib.check(rc, entry)
        ctx.plan, ctx.n_head, ctx.concat, ctx.head_is_scale = plan, n_head, concat, head_is_scale
        ctx.save_for_backward(values, head, rowstat, scale)
        return out

    @staticmethod
    def backward(ctx, d_out):
        values, head, rowstat, scale = ctx.saved_tensors
        plan, n_head = ctx.plan, ctx.n_head
        b, j, d = values.shape
        d_out = d_out.contiguous()
        _need_gpu(d_out)
        need_v, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_values = torch.empty((b, j, d), device=values.device, dtype=torch.float32) if need_v else None
        d_head = torch.empty((n_head,), device=values.device, dtype=torch.float32) if need_h else None
        work = _dscale_workspace(values.device, n_head) if need_h else None
        if need_v or need_h:
            io = _layer_io(values, head, n_head, ctx.head_is_scale, ctx.concat, False, rowstat, scale, d_out=d_out,
                           d_values=d_values, d_head=d_head, work=work)
            entry, geometry = _PosAttRagged._geometry(plan, "bwd")
            rc = getattr(_lib.lib(), entry)(
                *geometry, *io.values, *io.head, io.rowstat, 1 if plan.masked else 0, *io.d_out, *io.d_values, *io.d_head,
                _lib.ptr(plan.nbr_idx), _lib.ptr(plan.nbr_cnt), plan.nbr_cap, _lib.ptr(plan.rev_ptr), _lib.ptr(plan.rev_row), *io.tail)
            _lib.check(rc, entry)
        return d_values, d_head, None, None, None, None


class _PosAtt(torch.autograd.Function):
    """dist2att + convolution (+ the self-attention concat) as one op."""

    @staticmethod
    def forward(ctx, values, head, plan: MeshPlan, n_head: int, concat: bool, head_is_scale: bool,
                head_param=None, out_slot=None, coord_dims: int = 0, scale_in=None, out_bf16: bool = False, link=None,
                mesh_out=None, mesh_in=None):
        _need_gpu(values, head)
        ctx.math = _math_code()
        ctx.repro = reproducible_wanted()          # (d(values) from sorted lists, overflowed rows in row order, no rider)
        # the caller's mesh tensors arrive only when one of them requires grad (posatt_apply): then the layer keeps the
        # per-row / dense kernels, whose rowstat pit_posatt_dmesh reads in the backward
        ctx.mesh_grad = mesh_out is not None or mesh_in is not None
        ctx.mesh_same = mesh_out is mesh_in
        ctx.mesh_shapes = (tuple(mesh_out.shape) if mesh_out is not None else None,
                           tuple(mesh_in.shape) if mesh_in is not None else None)
        if ctx.mesh_grad:
            _check_mesh_grad(plan.metric)
            if coord_dims:
                raise RuntimeError("mesh gradients need the coordinate concat materialised (ops.materialize_coords)")
            out_bf16 = False
        out_bf16 = bool(out_bf16 and not concat and plan.nbr_idx is not None and ctx.math == MATH_MODES["bf16"])
        ctx.coord_dims = int(coord_dims)
        # masked layer over a coherently ordered mesh: the union-tile kernels (decided per kind of plan, MeshPlan.union_tiles)
        ctx.union = ATT_UNION if (plan.masked and plan.nbr_idx is not None and not coord_dims and n_head <= 2
                                  and values.shape[-1] % 8 == 0 and plan.union_tiles()) else 0
        # (the concat buffer arrives in a one-element list, not as a tensor argument: a tensor that is both an
        # input and the returned output would be re-materialised by autograd with a full copy)
        out_buf = out_slot[0].detach() if out_slot else None
        values = _row_view(values)
        b, j, d = values.shape
        d += int(coord_dims)                      # coordinate channels come from mesh_in inside the kernel (pit_hip.h)
        if j != plan.n_in:
            raise RuntimeError(f"inputs have {j} points but mesh_in has {plan.n_in}")
        if plan.mesh_batch not in (1, b):
            raise RuntimeError("mesh batch and input batch differ")
        head = head.detach().reshape(-1).contiguous()
        if head.numel() != n_head:
            raise RuntimeError("lmda must hold one value per head")
        # round 5: masked cross attention on a batch-free mesh pair with a slab plan and a width that is a multiple of 64 - the
        # union-tile contraction of csrc/pit_edge.hip (weights once per call, d_out read once in the backward): Vorticity / Cylinder
        ctx.uatt = None
        if UNION_ATT and not ctx.mesh_grad and not ctx.repro and not concat and not coord_dims and out_buf is None and _union_att_ok(plan, n_head, d, b, values):
            w = _new_decoder_weights(plan, head, scale_in, n_head, head_is_scale, True, patch=False)      # (Q too: 2 KB per slab)
            _launch_decoder_weights(w)
            out = torch.empty((b, plan.n_out, n_head * d), device=values.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
            sp, max_union = plan.slab_plan()[0], plan.slab_plan()[1]
            rc = _lib.lib().pit_union_att_fwd(ctypes.byref(sp), values.data_ptr(), values.stride(1), values.stride(0), b, n_head, d,
                                              w.pw.data_ptr(), out.data_ptr(), out.stride(1), out.stride(0), 1 if out_bf16 else 0,
                                              max_union, _lib.stream_ptr())
            _lib.check(rc, "pit_union_att_fwd")
            ctx.uatt = w
            ctx.plan, ctx.n_head, ctx.concat, ctx.head_is_scale = plan, n_head, concat, head_is_scale
            ctx.head_param = head_param
            ctx.union = 0
            ctx.save_for_backward(values, head, w.scale, w.scale)
            return out
        # round 6, bf16 mode: the processor's dense self-attention (locality 1.0) at hid 128 / 256 on bf16 MFMA with the values rounded
        # once per layer (csrc/pit_satt.hip)
        ctx.satt = None
        if not ctx.mesh_grad and _satt_pays(int(plan.n_in), int(n_head), int(d)) and concat and not coord_dims and plan.self_attn and not plan.masked and ctx.math == MATH_MODES["bf16"] \
                and values.dtype == torch.float32 and values.stride(1) % 4 == 0 and values.stride(0) % 4 == 0 and values.data_ptr() % 16 == 0 \
                and plan.sdim <= 3 and _lib.lib().pit_satt_supported(int(plan.n_in), int(n_head), int(d), int(b), int(plan.mesh_batch)):
            k_head, k_is_scale = (scale_in, True) if scale_in is not None else (head, head_is_scale)
            out = out_buf if out_buf is not None else torch.empty((b, plan.n_out, (n_head + 1) * d), device=values.device, dtype=torch.float32)
            # (the producing MLP chain may already have written bf16(values): link["x16"] - then no prep launch)
            x16 = link.get("x16") if (link is not None and out_buf is not None) else None
            x16_ready = x16 is not None and tuple(x16.shape) == (b * j, d) and x16.dtype == torch.bfloat16 and x16.is_contiguous()
            if not x16_ready:
                x16 = torch.empty((b, j, d), device=values.device, dtype=torch.bfloat16)
            rowstat = torch.empty((plan.mesh_batch, n_head, plan.n_out, 4), device=values.device, dtype=torch.float32)
            scale = torch.empty((n_head,), device=values.device, dtype=torch.float32)
            # the forward's rounded weights, kept as MFMA A-fragment tiles for the backward's d(values) (2 MB per sample and head at
            # Elasticity's 972 points)
            et = torch.empty((plan.mesh_batch, n_head, int(_lib.lib().pit_satt_tiles_elems(int(plan.n_in)))), device=values.device,
                             dtype=torch.bfloat16) if SATT_TILES else None
            rc = _lib.lib().pit_satt_fwd(plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_in, plan.sdim, plan.metric_id, plan.period,
                                         values.data_ptr(), values.stride(1), values.stride(0), b, d, k_head.data_ptr(), n_head,
                                         1 if k_is_scale else 0, x16.data_ptr(), out.data_ptr(), out.stride(1), out.stride(0), d,
                                         1 if out_buf is None else 0, rowstat.data_ptr(), scale.data_ptr(), _lib.ptr(et),
                                         1 if x16_ready else 0, _lib.stream_ptr())
            _lib.check(rc, "pit_satt_fwd")
            ctx.satt = x16
            ctx.satt_tiles = et
            # what the consuming MLP chain's backward needs to write this layer's G16 beside its d_x (posatt_apply hangs it on `out`)
            ctx.satt_link = link
            if link is not None:
                link.update(rowstat=rowstat, n_head=n_head, pts=int(j), mesh_batch=int(plan.mesh_batch), dim=int(d), batch=int(b), g16=None,
                            dx_ptr=None, dx_version=None)
            ctx.union = 0
            ctx.plan, ctx.n_head, ctx.concat, ctx.head_is_scale = plan, n_head, concat, head_is_scale
            ctx.head_param = head_param
            ctx.save_for_backward(values, head, rowstat, scale)
            return out
        width = (n_head + (1 if concat else 0)) * d
        copy_inputs = 1 if concat else 0
        if out_buf is not None:
            # the producer (mlp_apply(..., concat_heads=H)) already wrote `values` into columns [0, d) of this
            # buffer: the kernel only adds the head columns - no copy of the inputs (torch.cat of pit.py:44)
            out, copy_inputs = out_buf, 0
        else:
            out = torch.empty((b, plan.n_out, width), device=values.device,
                              dtype=torch.bfloat16 if out_bf16 else torch.float32)
        rowstat = torch.empty((plan.mesh_batch, n_head, plan.n_out, 4), device=values.device, dtype=torch.float32)
        scale = torch.empty((n_head,), device=values.device, dtype=torch.float32)
        # route 'host': `head` is lmda (autograd's input, the chain rule of the backward) but the kernels are
        # handed the scale c the host evaluated for it (scale_in); the backward gets it back through `scale`
        k_head, k_is_scale = (scale_in, True) if scale_in is not None else (head, head_is_scale)
        wjob = getattr(_STEP, "fwd_job", None)             # the processor's weights riding in this launch (early_block_weights)
        if wjob is not None:
            _STEP.fwd_job = None
        rc = _lib.lib().pit_posatt_fwd_job(
            plan.mesh_out.data_ptr(), plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_out, plan.n_in, plan.sdim,
            plan.metric_id, plan.period,
            values.data_ptr(), b, d, values.stride(1), values.stride(0),
            k_head.data_ptr(), n_head, 1 if k_is_scale else 0,
            _lib.ptr(plan.stats), plan.rank_w, 1 if plan.masked else 0, 1 if plan.self_attn else 0,
            out.data_ptr(), out.stride(1), out.stride(0), d if concat else 0, copy_inputs,
            rowstat.data_ptr(), scale.data_ptr(),
            _lib.ptr(plan.nbr_idx), _lib.ptr(plan.nbr_cnt), plan.nbr_cap, ctx.coord_dims,
            ctx.math | (IO_OUT_BF16 if out_bf16 else 0) | ctx.union, _lib.stream_ptr(),
            ctypes.cast(ctypes.pointer(wjob.job), ctypes.c_void_p) if wjob is not None else None)
        _lib.check(rc, "pit_posatt_fwd")
        ctx.plan, ctx.n_head, ctx.concat, ctx.head_is_scale = plan, n_head, concat, head_is_scale
        ctx.head_param = head_param
        ctx.save_for_backward(values, head, rowstat, scale)
        return out

    @staticmethod
    def backward(ctx, d_out):
        values, head, rowstat, scale = ctx.saved_tensors
        plan, n_head, concat = ctx.plan, ctx.n_head, ctx.concat
        b, j, dv = values.shape
        d = dv + ctx.coord_dims
        d_out = _row_view(d_out)
        _need_gpu_bf16_ok(d_out)
        io = IO_DOUT_BF16 if d_out.dtype == torch.bfloat16 else 0
        need_v, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        union = ctx.union
        if union:                                       # (the kernels' 16-byte row pieces: csrc/pit_posatt.hip union_ok / aligned_rows)
            k = 8 if io else 4
            if (values.data_ptr() | d_out.data_ptr()) % 16 or values.stride(1) % 4 or values.stride(0) % 4 \
                    or d_out.stride(1) % k or d_out.stride(0) % k:
                union = 0
        # d(values): from the union tiles (fp32 atomic adds: sums that differ in the last bits from run to run - not under
        # torch.use_deterministic_algorithms, nor with PIT_UNION_DV=lists), else from the transposed lists, built on demand
        repro = getattr(ctx, "repro", False)
        if need_v and not (union and UNION_DV != "lists" and not torch.are_deterministic_algorithms_enabled() and not repro):
            plan.ensure_reverse_lists()
        # reproducible mode: every key's range of the transposed lists in ascending row order (the order d(values) is summed in)
        rev_row = plan.sorted_reverse_lists() if (repro and need_v and plan.rev_ptr is not None) else plan.rev_row
        if repro and io:                            # (pit_posatt_overflow_dv_ordered reads an fp32 d_out)
            raise NotImplementedError("the reproducible mode takes an fp32 d_out only")
        ordered_lists = repro and need_v and plan.nbr_idx is not None and plan.masked and plan.rev_ptr is not None and not io
        d_values = torch.empty((b, j, dv), device=values.device, dtype=torch.float32) if need_v else None
        uatt, satt = ctx.uatt, getattr(ctx, "satt", None)
        # (the candidate-list / dense launch forms d(lmda) itself unless deferred; the other two leave it to the finishing kernel)
        hg = _HeadGrad(ctx.head_param, need_h, n_head, values.device, ctx.head_is_scale, shared_workspace=True,
                       kernel_finishes=uatt is None and satt is None)
        work = hg.work

        def launch(dv, dh, stream_ptr, job=None):
            rc = _lib.lib().pit_posatt_bwd(
                plan.mesh_out.data_ptr(), plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_out, plan.n_in,
                plan.sdim, plan.metric_id, plan.period,
                values.data_ptr(), b, d, values.stride(1), values.stride(0),
                head.data_ptr(), n_head, 1 if ctx.head_is_scale else 0, scale.data_ptr(),
                rowstat.data_ptr(), 1 if plan.masked else 0,
                d_out.data_ptr(), d_out.stride(1), d_out.stride(0), d if concat else 0,
                _lib.ptr(dv), dv.stride(1) if dv is not None else 0, dv.stride(0) if dv is not None else 0,
                1 if concat else 0,
                _lib.ptr(dh), hg.acc, work.data_ptr(),
                _lib.ptr(plan.nbr_idx), _lib.ptr(plan.nbr_cnt), plan.nbr_cap, 1 if ordered_lists else plan.lists_complete(),
                _lib.ptr(plan.rev_ptr), _lib.ptr(rev_row),
                ctypes.cast(ctypes.pointer(job[0]), ctypes.c_void_p) if job is not None else None,
                ctx.coord_dims, ctx.math | io | union, stream_ptr)
            _lib.check(rc, "pit_posatt_bwd")
            if ordered_lists:
                # the rows whose list overflowed (pit_posatt_bwd was told there are none: its pass adds with atomics), in row order
                rc = _lib.lib().pit_posatt_overflow_dv_ordered(
                    plan.mesh_out.data_ptr(), plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_out, plan.n_in,
                    plan.sdim, plan.metric_id, plan.period, b, d, head.data_ptr(), n_head, 1 if ctx.head_is_scale else 0,
                    scale.data_ptr(), rowstat.data_ptr(), d_out.data_ptr(), d_out.stride(1), d_out.stride(0), d if concat else 0,
                    dv.data_ptr(), dv.stride(1), dv.stride(0), plan.nbr_cnt.data_ptr(), plan.nbr_cap, ctx.coord_dims, stream_ptr)
                _lib.check(rc, "pit_posatt_overflow_dv_ordered")

        # an MLP's postponed weight-gradient reductions ride along - unless this is a candidate-list layer and the job is
        # LARGE (the decoder MLP's: inside that launch it costs more than a launch of its own, measured 34.7 vs 16.1 +
        # 15.7 us at Darcy b=8); left pending, the fused processor spreads it over its block launches (_Processor.backward)
        # or the next MLP backward / the end of the pass runs it
        carry = not (repro or (plan.nbr_idx is not None and _dw_pending_rows(values.device) >= BIG_RIDER_ROWS))
        fscale = scale                                   # (the scale c the finishing kernel's chain rule reads)
        if uatt is not None:                             # the union-tile backward: d_out read once, d(values) added from the tiles
            if carry:
                _dw_run_pending(values.device)           # (this launch carries nothing)
            if d_values is not None:
                d_values.zero_()
            sp, max_union = plan.slab_plan()[0], plan.slab_plan()[1]
            rc = _lib.lib().pit_union_att_bwd(ctypes.byref(sp), values.data_ptr(), values.stride(1), values.stride(0), b, n_head, dv,
                                              uatt.pw.data_ptr(), uatt.qw.data_ptr(), d_out.data_ptr(), d_out.stride(1), d_out.stride(0),
                                              1 if io else 0, _lib.ptr(d_values), d_values.stride(1) if d_values is not None else 0,
                                              d_values.stride(0) if d_values is not None else 0, work.data_ptr() if need_h else None,
                                              max_union, _lib.stream_ptr())
            _lib.check(rc, "pit_union_att_bwd")
            fscale = uatt.scale
        elif satt is not None:                           # dense self-attention on bf16 MFMA (csrc/pit_satt.hip)
            job = _dw_take(values.device) if carry else None
            if job is not None and not SATT_DW_RIDER:    # (else carried by the launch below; `job[1]` keeps its tensors alive)
                _dw_run(job)
                job = None
            if d_out.dtype != torch.float32 or d_out.stride(1) % 4 or d_out.stride(0) % 4 or d_out.data_ptr() % 16:
                d_out = d_out.float().contiguous()
            lk = getattr(ctx, "satt_link", None)
            g16 = lk.get("g16") if lk is not None else None
            g16_ready = _handoff_g16_ready(lk, d_out, (b, n_head, j, dv))
            if lk is not None:
                lk["g16"] = None                         # (consumed)
            if not g16_ready:
                g16 = torch.empty((b, n_head, j, dv), device=values.device, dtype=torch.bfloat16)
            rc = _lib.lib().pit_satt_bwd(plan.mesh_in.data_ptr(), plan.mesh_batch, plan.n_in, plan.sdim, plan.metric_id, plan.period,
                                         b, dv, scale.data_ptr(), n_head, rowstat.data_ptr(), satt.data_ptr(), g16.data_ptr(),
                                         d_out.data_ptr(), d_out.stride(1), d_out.stride(0), dv,
                                         _lib.ptr(d_values), d_values.stride(1) if d_values is not None else 0,
                                         d_values.stride(0) if d_values is not None else 0, 1,
                                         work.data_ptr() if need_h else None, _lib.ptr(getattr(ctx, "satt_tiles", None)),
                                         1 if g16_ready else 0, ctypes.byref(job[0]) if job is not None else None, _lib.stream_ptr())
            _lib.check(rc, "pit_satt_bwd")
        else:
            launch(d_values, hg.d_head, _lib.stream_ptr(), _dw_take(values.device) if carry else None)
        # (forward's inputs: values, head, then plan, n_head, concat, head_is_scale, head_param, out_slot, coord_dims, scale_in,
        # out_bf16, link - and the two meshes)
        return (d_values, hg.finish(head, fscale)) + (None,) * 10 + _mesh_grads(ctx, values, head, rowstat, scale, d_out)


# Where the head scale c = tan(0.25*pi*(1-1e-7)*(1+sin(lmda))) (pit.py:48) is evaluated.
#   "device" (default): inside the kernels, through fp64 with the reference's fp32 roundings - no host
#       sync, hipGraph-capturable.  ATen-CPU evaluates sin/tan with MKL VML (high-accuracy mode, NOT
#       correctly rounded, kernels chosen by the host CPU), so this c differs from the reference's by
#       1 ulp or more for ~2 % of lmda; on regular grids that can move a tie shell across the quantile
#       threshold (DESIGN.md section 2 quantifies it).
#   "host": the reference's own op sequence on the HOST CPU (torch.sin / torch.tan on a CPU copy of
#       lmda, i.e. bit-for-bit what pit.py:48 computes on that machine), injected into the kernels as
#       the scale and CACHED per lmda version (host_head_scale): one device->host copy per layer when
#       lmda changed, none while it is frozen - evaluation of a checkpoint and forward+backward with
#       frozen lmda are sync-free and hipGraph-capturable after one eager call.  d(lmda) is the kernels'
#       closed-form chain rule (1+c^2)*K*cos(lmda) in fp64 with that exact c.  A captured step that
#       UPDATES lmda (optimizer inside the graph) is refused: use 'device' there.
HEAD_SCALE_ROUTES = ("device", "host")
_ROUTE = threading.local()
_DEFAULT_ROUTE = os.environ.get("PIT_HEAD_SCALE_ROUTE", "device")
if _DEFAULT_ROUTE not in HEAD_SCALE_ROUTES:
    raise ValueError(f"PIT_HEAD_SCALE_ROUTE must be one of {HEAD_SCALE_ROUTES}, got {_DEFAULT_ROUTE!r}")


def set_head_scale_route(route: str) -> None:
    if route not in HEAD_SCALE_ROUTES:
        raise ValueError(f"head-scale route must be one of {HEAD_SCALE_ROUTES}, got {route!r}")
    _ROUTE.route = route


def get_head_scale_route() -> str:
    """Per-thread route; the process default is 'device' unless PIT_HEAD_SCALE_ROUTE=host is set in the environment
    (exact reproduction of a reference checkpoint by an unmodified script)."""
    return getattr(_ROUTE, "route", _DEFAULT_ROUTE)


class head_scale_route:
    """`with ops.head_scale_route('host'): ...` - scoped set_head_scale_route."""

    def __init__(self, route: str):
        self.route, self.prev = route, None

    def __enter__(self):
        self.prev = get_head_scale_route()
        set_head_scale_route(self.route)
        return self

    def __exit__(self, *exc):
        set_head_scale_route(self.prev)
        return False


# Anything that rewrites parameters behind autograd's back (raw-pointer writers: ddp.FlatAdam, a replayed
# hipGraph that contains an optimizer step) bumps this epoch through ``parameters_changed()``; together with the
# tensor's own version counter (bumped by every torch in-place op: torch.optim, load_state_dict, copy_) it keys the
# cached host-evaluated head scales below.
_PARAM_EPOCH = [0]
_HOSTC_CAPTURE = {"used": False, "log": []}      # scales consumed under the running stream capture: (lmda, version)
HOST_SCALE_EVALUATIONS = [0]                     # device->host round trips taken by host_head_scale (tests read it)


def parameters_changed() -> None:
    """Tell the operators that parameter VALUES were rewritten without a torch in-place op (fused optimizer
    through raw pointers, graph replay of a captured optimizer step): cached head scales are dropped.  Inside a
    stream capture that already consumed a cached scale this is an error - replays would change lmda while the
    graph keeps feeding the kernels the scale of the lmda it was captured with."""
    if _capturing() and _HOSTC_CAPTURE["used"]:
        raise RuntimeError("head-scale route 'host' is exact for a FROZEN lmda only: this capture consumed a "
                           "host-evaluated scale and now updates the parameters inside the same graph; capture "
                           "training steps that include the optimizer with the 'device' route")
    _PARAM_EPOCH[0] += 1


def host_head_scale(lmda: torch.Tensor) -> torch.Tensor:
    """c(lmda) (n_head floats on lmda's device) by the reference's own op sequence on the HOST CPU - bit-for-bit
    what pit.py:48 evaluates on this machine - cached on the tensor per (version counter, storage, epoch):
    one device->host copy when lmda changed, none while it is frozen (evaluation, fwd+bwd benchmarks), so a step
    with frozen lmda is sync-free and can be captured into a hipGraph after one eager call.  A miss under capture
    raises: the copy would synchronise."""
    key = (lmda._version, lmda.data_ptr(), _PARAM_EPOCH[0], lmda.device.index)
    ent = getattr(lmda, "_pit_host_c", None)
    if ent is None or ent[0] != key:
        if _capturing():
            raise RuntimeError("head-scale route 'host' cannot be captured into a hipGraph for an lmda whose current "
                               "value has no host-evaluated scale yet (that needs a device->host copy): it is exact "
                               "for a FROZEN lmda only - run the step once eagerly with this route first; if an "
                               "optimizer updates lmda every step, capture with the 'device' route")
        HOST_SCALE_EVALUATIONS[0] += 1
        host = lmda.detach().reshape(-1).cpu()
        c = torch.tan(0.25 * math.pi * (1 - 1e-7) * (1.0 + torch.sin(host)))
        ent = (key, c.to(lmda.device))
        lmda._pit_host_c = ent
    if _capturing():
        _HOSTC_CAPTURE["used"] = True
        _HOSTC_CAPTURE["log"].append((lmda, lmda._version))
        _pin(ent[1])
    else:
        _HOSTC_CAPTURE["used"] = False
        _HOSTC_CAPTURE["log"].clear()
    return ent[1]


def assert_frozen_since_capture() -> None:
    """After a capture (engine.TrainStep.capture): every lmda whose host-evaluated scale went into the graph must
    not have been modified by the captured work (a torch optimizer inside the graph bumps its version)."""
    log, _HOSTC_CAPTURE["log"] = _HOSTC_CAPTURE["log"], []
    _HOSTC_CAPTURE["used"] = False
    for lmda, version in log:
        if lmda._version != version:
            raise RuntimeError("head-scale route 'host' is exact for a FROZEN lmda only, but the captured step "
                               "modified lmda (an optimizer inside the graph): capture it with the 'device' route")


def _concat_buffer_of(values: torch.Tensor, n_out: int, n_head: int):
    """The concat buffer a producer attached to ``values`` (mlp_apply(..., concat_heads=H)), if ``values`` really
    is its first-columns view with the layout this layer needs; consumed once (a second consumer gets a copy)."""
    buf = getattr(values, "_pit_concat", None)
    if buf is None:
        return None
    values._pit_concat = None
    b, j, d = values.shape
    w = (1 + n_head) * d
    ok = (buf.dim() == 3 and tuple(buf.shape) == (b, n_out, w) and j == n_out and buf.is_contiguous()
          and values.data_ptr() == buf.data_ptr() and tuple(values.stride()) == (n_out * w, w, 1))
    return buf if ok else None


def tag_coords(func: torch.Tensor, mesh_in: torch.Tensor) -> torch.Tensor:
    """``func`` (b, J, C) as the non-coordinate channels of the encoder input ``cat((tile(mesh_in), func), -1)``
    that the fixed-mesh task forwards build (train_darcy.py:51-55): returns an alias of ``func`` carrying the mesh,
    so that a cross-attention layer on candidate lists reads the coordinate channels from ``mesh_in`` itself instead
    of a materialised concat (``materialize_coords`` builds the concat for every other consumer)."""
    out = func.view_as(func)                     # a fresh tensor object: never tag the caller's own tensor
    out._pit_coords = mesh_in
    return out


def materialize_coords(func: torch.Tensor) -> torch.Tensor:
    """The explicit concat for a tensor tagged by ``tag_coords`` (identity for any other tensor)."""
    mesh = getattr(func, "_pit_coords", None)
    if mesh is None:
        return func
    return torch.cat((mesh.reshape(1, -1, mesh.shape[-1]).expand(func.shape[0], -1, -1), func), -1)


@torch.compiler.disable
def posatt_apply(values: torch.Tensor, lmda: torch.Tensor, plan: MeshPlan, n_head: int, concat: bool,
                 head_is_scale: bool = False, coord_dims: int = 0, out_bf16: bool = False,
                 mesh_out: Optional[torch.Tensor] = None, mesh_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b,n,h*D+d] = sum_j softmax_j(-c_h m[n,j] | quantile mask)[n,j] * values[b,j,d]
    (pit.py:46-57); with ``concat`` the inputs are prepended (pit.py:44).  ``lmda`` is the
    (H,1,1) parameter, or the scale c itself when ``head_is_scale`` (tests inject it).
    ``coord_dims`` > 0: the first coord_dims value channels are the key coordinates (plan.mesh_in), ``values`` holds
    the others (candidate-list layers only, see pit_hip.h).
    ``mesh_out`` / ``mesh_in``: the caller's mesh tensors (those ``plan`` was built from).  When grad mode is on and one of
    them requires grad they become inputs of the op and receive d(mesh) from pit_posatt_dmesh (Euclidean metric, fp32 mode;
    NotImplementedError otherwise); otherwise they are ignored.
    Opaque to torch.compile (dynamo runs it eagerly: raw pointers cross a ctypes boundary)."""
    if plan.ragged():                              # ragged batch: the pit_posatt_ragged_* entries, every layer on its own
        if mesh_grad_wanted(mesh_out, mesh_in):
            raise NotImplementedError("lengths with a mesh that requires grad: mesh gradients are not implemented for ragged batches")
        if get_math_mode() != "fp32":
            raise NotImplementedError("lengths in the bf16 math mode: ragged batches run in the fp32 math mode only")
        if coord_dims:
            raise RuntimeError("ragged batches need the coordinate concat materialised (ops.materialize_coords)")
        return _PosAttRagged.apply(values, lmda.reshape(-1), plan, n_head, concat, head_is_scale)
    meshes = ()
    reproducible_wanted()                          # (bf16 mode: refused here, before anything is launched)
    if mesh_grad_wanted(mesh_out, mesh_in):
        _check_mesh_grad(plan.metric)
        meshes = (mesh_out, mesh_in)
    out_buf = _concat_buffer_of(values, plan.n_out, n_head) if concat else None
    slot = [out_buf] if out_buf is not None else None
    param = lmda if isinstance(lmda, torch.nn.Parameter) else None
    c = host_head_scale(lmda) if (not head_is_scale and get_head_scale_route() == "host") else None
    # the hand-offs between a dense self-attention layer on csrc/pit_satt.hip and the MLP chains either side of it (bf16 mode):
    # bf16(values) from the producing chain, and - on the way back - G16 from the consuming chain's backward
    link = {"x16": _handoff_x16(values)} if concat else None
    out = _PosAtt.apply(values, lmda.reshape(-1), plan, n_head, concat, head_is_scale, param, slot, coord_dims, c,
                        out_bf16, link, *meshes)
    if link is not None and link.get("rowstat") is not None:
        out._pit_satt = link
    elif concat and plan.self_attn and not plan.masked and plan.nbr_idx is None and not coord_dims:
        out._pit_dense_att = True                # (the MLP behind it may postpone its weight-gradient reductions for this layer's backward)
    return out


# ---- position attention on caller-supplied squared distances (csrc/pit_distmat.hip; metric.py) ----------------------------------
def _check_dist_mode() -> None:
    if get_math_mode() != "fp32":
        raise NotImplementedError("attention on a caller-supplied distance matrix runs in the fp32 math mode only (set_math_mode('fp32'))")


def check_dist_shapes(m_dist, values, concat: bool) -> None:
    """Shape refusals of a layer on a distance matrix, raised before the device check and before anything is launched."""
    if not torch.is_tensor(m_dist) or m_dist.dim() not in (2, 3):
        raise ValueError("m_dist must be an (N, J) or (b, N, J) tensor of squared distances")
    if not torch.is_tensor(values) or values.dim() != 3:
        raise ValueError("inputs must be a (batch, J, channels) tensor")
    if values.shape[1] != m_dist.shape[-1]:
        raise ValueError(f"inputs have {values.shape[1]} points but the distance matrix has {m_dist.shape[-1]} columns")
    if m_dist.dim() == 3 and m_dist.shape[0] != values.shape[0]:
        raise ValueError(f"the distance matrix holds {m_dist.shape[0]} samples, the inputs {values.shape[0]}")
    if concat and m_dist.shape[-2] != m_dist.shape[-1]:
        raise ValueError("the self-attention form needs a square distance matrix")


class DistPlan:
    """Selection statistics of a caller-supplied matrix of squared distances ``m_dist`` - (N, J), shared by the whole batch, or
    (b, N, J), one per sample - under ``locality`` (pit_distmat_select_fwd: what the sort inside torch.quantile would find,
    pit.py:49).  Keeps a detached view of the caller's tensor (a copy only where its rows are not contiguous); precondition:
    finite and >= 0, not checked."""

    def __init__(self, m_dist: torch.Tensor, locality: float):
        _check_dist_mode()
        if not torch.is_tensor(m_dist) or m_dist.dim() not in (2, 3):
            raise ValueError("m_dist must be an (N, J) or (b, N, J) tensor of squared distances")
        if m_dist.dtype != torch.float32:
            raise ValueError(f"m_dist must be fp32, got {m_dist.dtype}")
        if 0 in m_dist.shape:
            raise ValueError(f"m_dist has an empty axis: {tuple(m_dist.shape)}")
        if not (0.0 <= float(locality) <= 1.0):
            raise ValueError(f"locality must lie in [0, 1], got {locality}")
        _need_gpu(m_dist)
        self.source = m_dist.detach()                      # (keeps the caller's storage - and with it its address - alive)
        m = self.source if m_dist.dim() == 3 else self.source.unsqueeze(0)
        mb, n, j = m.shape
        if m.stride(2) != 1 or (n > 1 and m.stride(1) < j) or (mb > 1 and m.stride(0) < (n - 1) * m.stride(1) + j):
            m = m.contiguous()
        self.m = m
        self.mesh_batch, self.n_out, self.n_in = int(mb), int(n), int(j)
        self.ld_m = int(m.stride(1)) if n > 1 else int(j)
        self.m_bstride = int(m.stride(0)) if mb > 1 else 0
        self.locality = float(locality)
        self.masked = self.locality < 1.0
        self.rank_k, self.rank_w = quantile_rank(self.locality, self.n_in)
        self.stats = torch.empty((3, mb * n), device=m.device, dtype=torch.float32)
        rc = _lib.lib().pit_distmat_select_fwd(m.data_ptr(), self.ld_m, self.m_bstride, self.mesh_batch, self.n_out, self.n_in,
                                               self.rank_k, 1, self.stats.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_distmat_select_fwd")
        if _capturing():
            _pin(self)

    REFUSALS = ("inputs have {j} points but the distance matrix has {n_in} columns", "distance-matrix batch and input batch differ",
                "the self-attention form needs a square distance matrix")
    NOT_THE_SOURCE = "m_dist is not the matrix the plan was built from"

    def source_grad_shape(self):
        return (self.mesh_batch, self.n_out, self.n_in)

    def _geometry(self):
        return (self.m.data_ptr(), self.ld_m, self.m_bstride, self.n_out, self.n_in)

    def launch_fwd(self, io) -> None:
        rc = _lib.lib().pit_distmat_fwd(*self._geometry(), *io.values, *io.head, self.stats.data_ptr(), self.rank_w, 1 if self.masked else 0,
                                        *io.out, *io.tail)
        _lib.check(rc, "pit_distmat_fwd")

    def launch_bwd(self, io, grads) -> None:
        """``grads``: d_source (None: not wanted), the forward's result with it, and whether d(values) is wanted."""
        L = _lib.lib()
        a_ws = None
        if grads.d_source is not None:
            a_ws = torch.empty(((L.pit_distmat_bwd_workspace(io.batch, self.n_out, io.n_head) + 3) // 4,), device=self.m.device, dtype=torch.float32)
        rc = L.pit_distmat_bwd(*self._geometry(), *io.values, *io.head, io.rowstat, 1 if self.masked else 0, *io.d_out, *io.d_values, *io.d_head,
                               _lib.ptr(grads.d_source), *_lib.saved_out_args(grads.out), _lib.ptr(a_ws), *io.tail)
        _lib.check(rc, "pit_distmat_bwd")


class _PosAttSupplied(torch.autograd.Function):
    """pit.py:48-57 (+ the concat of :44) on supplied squared distances - a DistPlan (pit_distmat_fwd / _bwd) or a ListPlan
    (pit_distlist_fwd / _bwd) - as one autograd node; the plan places its geometry around the shared argument groups.
    ``source`` (the caller's m_dist / sqd) arrives only when it requires grad and then receives d loss / d source in its own
    shape (for lists: 0 at padding)."""

    @staticmethod
    def forward(ctx, values, head, plan, n_head: int, concat: bool, head_is_scale: bool, scale_in=None, source=None):
        values, head, out, rowstat, scale = _layer_outputs(values, head, plan, n_head, concat, plan.REFUSALS, True)
        # route 'host': the kernels are handed the scale the host evaluated for lmda (scale_in), as in _PosAtt
        k_head, k_is_scale = (scale_in, True) if scale_in is not None else (head, head_is_scale)
        plan.launch_fwd(_layer_io(values, k_head, n_head, k_is_scale, concat, True, rowstat, scale, out=out))
        ctx.plan, ctx.n_head, ctx.concat, ctx.head_is_scale = plan, n_head, concat, head_is_scale
        ctx.source_shape = tuple(source.shape) if source is not None else None
        # (d(source) needs a_i = g_i . out_i: the result itself is kept then)
        ctx.save_for_backward(values, head, rowstat, scale, *((out,) if source is not None else ()))
        return out

    @staticmethod
    def backward(ctx, d_out):
        values, head, rowstat, scale = ctx.saved_tensors[:4]
        plan, n_head = ctx.plan, ctx.n_head
        b, j, d = values.shape
        if d_out.dtype != torch.float32:
            d_out = d_out.float()
        d_out = _row_view(d_out)
        _need_gpu(d_out)
        need_v, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_s = ctx.source_shape is not None and ctx.needs_input_grad[7]
        dev = values.device
        d_values = torch.empty((b, j, d), device=dev, dtype=torch.float32) if need_v else None
        d_head = torch.empty((n_head,), device=dev, dtype=torch.float32) if need_h else None
        work = _dscale_workspace(dev, n_head) if need_h else None
        d_source = torch.empty(plan.source_grad_shape(), device=dev, dtype=torch.float32) if need_s else None
        if need_v or need_h or need_s:
            io = _layer_io(values, head, n_head, ctx.head_is_scale, ctx.concat, True, rowstat, scale, d_out=d_out,
                           d_values=d_values, d_head=d_head, work=work)
            plan.launch_bwd(io, types.SimpleNamespace(d_source=d_source, out=ctx.saved_tensors[4] if need_s else None, need_values=need_v))
        return d_values, d_head, None, None, None, None, None, (d_source.view(ctx.source_shape) if need_s else None)


def _posatt_supplied_apply(values, lmda, plan, n_head: int, concat: bool, head_is_scale: bool, source):
    _check_dist_mode()
    if _capturing():
        _pin(plan)                                 # its buffers' addresses are now baked into a hipGraph: never release them
    values = materialize_coords(values)
    c = host_head_scale(lmda) if (not head_is_scale and get_head_scale_route() == "host") else None
    extra = ()
    if source is not None and torch.is_grad_enabled() and source.requires_grad:
        shape = plan.source_grad_shape()
        if tuple(source.shape)[-2:] != shape[1:] or source.numel() != shape[0] * shape[1] * shape[2]:
            raise ValueError(plan.NOT_THE_SOURCE)
        extra = (source,)
    return _PosAttSupplied.apply(values, lmda.reshape(-1), plan, n_head, concat, head_is_scale, c, *extra)


@torch.compiler.disable
def posatt_dist_apply(values: torch.Tensor, lmda: torch.Tensor, plan: DistPlan, n_head: int, concat: bool = False,
                      head_is_scale: bool = False, m_dist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``posatt_apply`` for squared distances the caller supplies: out[b,n,h*D+d] = sum_j softmax_j(-c_h m[n,j] | quantile
    mask)[n,j] * values[b,j,d] (pit.py:48-57) with ``m`` = the matrix ``plan`` was built from; ``concat`` prepends the inputs
    (pit.py:44).  ``m_dist``: the caller's own tensor (the one ``plan`` was built from); when grad mode is on and it requires
    grad it becomes an input of the node and receives d loss / d m - autograd then carries the gradient on through whatever torch
    code formed the distances, for any metric.  fp32 math mode only; head-scale routes as in ``posatt_apply``."""
    return _posatt_supplied_apply(values, lmda, plan, n_head, concat, head_is_scale, m_dist)


# ---- the same layer on candidate lists of caller-supplied squared distances (csrc/pit_distlist.hip; metric.py) -------------------
def list_capacity(locality: float, n_in: int) -> int:
    """Least width of the candidate lists of a layer of ``locality`` over ``n_in`` keys: k + 2 slots (the selection needs
    m_(k) and m_(k+1) and the row's tie at m_(k+1)), 1 without a mask."""
    if float(locality) >= 1.0:
        return 1
    return quantile_rank(float(locality), int(n_in))[0] + 2


def check_list_shapes(idx, sqd, values, concat: bool) -> None:
    """Shape and dtype refusals of a layer on candidate lists, raised before the device check and before anything is launched."""
    if not torch.is_tensor(idx) or not torch.is_tensor(sqd) or idx.dim() not in (2, 3):
        raise ValueError("idx and sqd must be (N, K) or (b, N, K) tensors: the keys and squared distances of each row's candidates")
    if tuple(idx.shape) != tuple(sqd.shape):
        raise ValueError(f"idx and sqd must have the same shape, got {tuple(idx.shape)} and {tuple(sqd.shape)}")
    if idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"idx must be int32 or int64, got {idx.dtype}")
    if sqd.dtype != torch.float32:
        raise ValueError(f"sqd must be fp32, got {sqd.dtype}")
    if 0 in idx.shape:
        raise ValueError(f"the lists have an empty axis: {tuple(idx.shape)}")
    if values is None:
        return
    if not torch.is_tensor(values) or values.dim() != 3:
        raise ValueError("inputs must be a (batch, J, channels) tensor")
    if idx.dim() == 3 and idx.shape[0] != values.shape[0]:
        raise ValueError(f"the lists hold {idx.shape[0]} samples, the inputs {values.shape[0]}")
    if concat and idx.shape[-2] != values.shape[1]:
        raise ValueError(f"the self-attention form needs one list per input point (N == J): {idx.shape[-2]} lists, {values.shape[1]} points")


class SharedListLengthsError(ValueError, NotImplementedError):
    """Lengths with (N, K) lists shared by the batch: a ValueError - the combination has no meaning, one list set cannot follow
    per-sample key counts - that callers written against the earlier blanket refusal of lengths (NotImplementedError) still catch."""


def check_list_lengths(idx, len_out, len_in) -> None:
    """What lengths on candidate lists do not cover, refused before the device check and before anything is launched."""
    if len_out is None and len_in is None:
        return
    if idx.dim() != 3:
        raise SharedListLengthsError("lengths need per-sample (b, N, K) lists: lists shared by the batch have no per-sample length")
    for name, given in (("len_out", len_out), ("len_in", len_in)):
        if given is None:
            continue
        if torch.is_tensor(given) and given.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be an int32 or int64 tensor, got {given.dtype}")
        count = given.numel() if torch.is_tensor(given) else len(given)
        if count != idx.shape[0]:
            raise ValueError(f"{name} must hold one entry per sample: {count} entries for a batch of {idx.shape[0]}")


class ListPlan:
    """Candidate lists ``(idx, sqd)`` - (N, K), shared by the whole batch, or (b, N, K) - of a layer of ``locality`` over
    ``n_in`` keys: an int32 copy of the keys, a detached view of the distances, the selection statistics over the valid slots
    (pit_distlist_select_fwd; the rank comes from ``n_in``, not from K) and - built when a backward first asks for it - the
    transposed index that d(values) runs over.  A slot whose key is outside [0, n_in) is padding.  Preconditions, not checked
    (a check would synchronise): valid distances finite and >= 0, no key twice in a row, at least k + 2 valid slots per row of a
    masked layer.

    ``len_out`` / ``len_in`` (either; ``as_lengths`` forms): a RAGGED batch on per-sample (b, N, K) lists - sample s has len_out[s]
    rows and len_in[s] keys; the plan keeps the two int32 device tensors (a captured step overwrites them in place) and a device
    array ``rank_w`` the selection fills per sample, and runs the pit_distlist_*_ragged_* entries.  ``n_in`` stays the padded
    width: the list width is checked against its rank, which bounds every sample's, and the transposed index is built against
    it from the keys alone, so it outlives any change of the lengths."""

    def __init__(self, idx: torch.Tensor, sqd: torch.Tensor, n_in: int, locality: float, len_out=None, len_in=None):
        _check_dist_mode()
        check_list_shapes(idx, sqd, None, False)
        self.ragged = len_out is not None or len_in is not None
        check_list_lengths(idx, len_out, len_in)
        if not (0.0 <= float(locality) <= 1.0):
            raise ValueError(f"locality must lie in [0, 1], got {locality}")
        n_in = int(n_in)
        if n_in <= 0:
            raise ValueError(f"n_in must be positive, got {n_in}")
        n, cap = int(idx.shape[-2]), int(idx.shape[-1])
        need = list_capacity(locality, n_in)
        if cap < need:
            raise ValueError(f"lists of {cap} slots are too narrow for locality {locality} over {n_in} keys: "
                             f"list_capacity gives {need} (k + 2)")
        if cap > LIST_MAX_CAP:
            raise ValueError(f"lists of {cap} slots: at most {LIST_MAX_CAP} are supported")
        if n * cap >= 2 ** 31:
            raise ValueError(f"N * K = {n * cap} does not fit 31 bits")
        _need_gpu(sqd)
        if idx.device != sqd.device:
            raise RuntimeError(f"idx lives on {idx.device}, sqd on {sqd.device}")
        self.len_out = None if len_out is None else as_lengths(len_out, sqd.device, int(idx.shape[0]))
        self.len_in = None if len_in is None else as_lengths(len_in, sqd.device, int(idx.shape[0]))
        self.source_idx, self.source = idx, sqd.detach()    # (keep the caller's storages - and with them their addresses - alive)
        i3 = idx.detach() if idx.dim() == 3 else idx.detach().unsqueeze(0)
        if i3.dtype != torch.int32:
            i3 = i3.clamp(-1, n_in).to(torch.int32)         # (every out-of-range key is padding: -1 and n_in stand for them all)
        self.idx = i3.contiguous()
        s3 = self.source if sqd.dim() == 3 else self.source.unsqueeze(0)
        self.sqd = s3.contiguous()
        self.mesh_batch, self.n_out, self.cap, self.n_in = int(i3.shape[0]), n, cap, n_in
        self.ld = cap
        self.bstride = n * cap if self.mesh_batch > 1 else 0
        self.locality = float(locality)
        self.masked = self.locality < 1.0
        self.rank_k, self.rank_w = quantile_rank(self.locality, n_in)
        self.stats = torch.empty((3, self.mesh_batch * n), device=sqd.device, dtype=torch.float32)
        self.rank_w_dev = torch.empty((self.mesh_batch,), device=sqd.device, dtype=torch.float32) if self.ragged else None
        self._rev = None
        self.refresh()

    def refresh(self) -> None:
        """Run the selection on what ``sqd`` holds NOW: for a caller that overwrites the distances in place (the keys unchanged) -
        one launch, no allocation, so it can be part of a captured step.  Without a mask only the row minima are computed."""
        src = self.source if self.source.dim() == 3 else self.source.unsqueeze(0)
        if self.sqd.data_ptr() != src.data_ptr():
            self.sqd.copy_(src)                             # (the caller's tensor was not contiguous: the plan works on a copy)
        if self.ragged:                                     # (the rank of every sample is formed on the device from its length)
            rc = _lib.lib().pit_distlist_select_ragged_fwd(self.idx.data_ptr(), self.sqd.data_ptr(), self.ld, self.bstride, self.cap,
                                                           self.mesh_batch, self.n_out, self.n_in, self.locality, 1 if self.masked else 0,
                                                           _lib.ptr(self.len_out), _lib.ptr(self.len_in), self.stats.data_ptr(),
                                                           self.rank_w_dev.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "pit_distlist_select_ragged_fwd")
            if _capturing():
                _pin(self)
            return
        rc = _lib.lib().pit_distlist_select_fwd(self.idx.data_ptr(), self.sqd.data_ptr(), self.ld, self.bstride, self.cap, self.mesh_batch,
                                                self.n_out, self.n_in, self.rank_k if self.masked else 0, 1 if self.masked else 0,
                                                self.stats.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_distlist_select_fwd")
        if _capturing():
            _pin(self)

    def transposed(self):
        """(rev_ptr, rev_pos, chunk_ptr, chunk_key) of pit_distlist_bwd, by torch integer ops that do not synchronise: a stable
        sort of the flattened keys (padding clamped to n_in, so it sorts behind every key) gives, per key, its listing slots
        row * K + slot in ascending order; searchsorted gives the range starts.  Any n_in."""
        if self._rev is None:
            mb, j, dev = self.mesh_batch, self.n_in, self.idx.device
            flat = self.idx.reshape(mb, -1)
            keys = torch.where((flat >= 0) & (flat < j), flat, torch.full_like(flat, j))
            skeys, order = torch.sort(keys, dim=1, stable=True)
            probe = torch.arange(j + 1, device=dev, dtype=torch.int32).unsqueeze(0).expand(mb, -1).contiguous()
            rev_ptr = torch.searchsorted(skeys, probe, right=False).to(torch.int32)
            cnt = rev_ptr[:, 1:] - rev_ptr[:, :-1]
            chunk = _lib.DISTLIST_CHUNK
            nch = torch.where(cnt > chunk, (cnt + (chunk - 1)) // chunk, torch.zeros_like(cnt))
            ends = torch.cumsum(nch, dim=1)
            chunk_ptr = torch.cat((torch.zeros((mb, 1), device=dev, dtype=ends.dtype), ends), dim=1).to(torch.int32).contiguous()
            slots = _lib.distlist_chunk_slots(self.n_out, self.cap)
            probe = torch.arange(slots, device=dev, dtype=ends.dtype).unsqueeze(0).expand(mb, -1).contiguous()
            chunk_key = torch.searchsorted(ends.contiguous(), probe, right=True).to(torch.int32)
            self._rev = (rev_ptr.contiguous(), order.to(torch.int32).contiguous(), chunk_ptr, chunk_key.contiguous())
        return self._rev

    REFUSALS = ("inputs have {j} points but the lists were planned for {n_in} keys", "list batch and input batch differ",
                "the self-attention form needs one list per input point")
    NOT_THE_SOURCE = "sqd is not the tensor the plan was built from"

    def source_grad_shape(self):
        return (self.mesh_batch, self.n_out, self.cap)

    def _geometry(self):
        return (self.idx.data_ptr(), self.sqd.data_ptr(), self.ld, self.bstride, self.cap, self.n_out, self.n_in)

    def launch_fwd(self, io) -> None:
        if self.ragged:
            rc = _lib.lib().pit_distlist_ragged_fwd(*self._geometry(), *io.values, *io.head, self.stats.data_ptr(), self.rank_w_dev.data_ptr(),
                                                    1 if self.masked else 0, _lib.ptr(self.len_out), _lib.ptr(self.len_in), *io.out, *io.tail)
            _lib.check(rc, "pit_distlist_ragged_fwd")
            return
        rc = _lib.lib().pit_distlist_fwd(*self._geometry(), *io.values, *io.head, self.stats.data_ptr(), self.rank_w, 1 if self.masked else 0,
                                         *io.out, *io.tail)
        _lib.check(rc, "pit_distlist_fwd")

    def launch_bwd(self, io, grads) -> None:
        """``grads``: as DistPlan.launch_bwd; d(values) runs over the transposed index and a workspace of partial rows."""
        L = _lib.lib()
        rev, dv_ws = (None, None, None, None), None
        if grads.need_values:
            rev = self.transposed()
            dv_ws = torch.empty(((L.pit_distlist_bwd_workspace(io.batch, self.n_out, self.cap, io.dim) + 3) // 4,), device=self.idx.device,
                                dtype=torch.float32)
        if self.ragged:
            rc = L.pit_distlist_ragged_bwd(*self._geometry(), *io.values, *io.head, io.rowstat, 1 if self.masked else 0, _lib.ptr(self.len_out),
                                           _lib.ptr(self.len_in), *io.d_out, *io.d_values, *io.d_head, _lib.ptr(grads.d_source),
                                           *_lib.saved_out_args(grads.out), *(_lib.ptr(t) for t in rev), _lib.ptr(dv_ws), *io.tail)
            _lib.check(rc, "pit_distlist_ragged_bwd")
            return
        rc = L.pit_distlist_bwd(*self._geometry(), *io.values, *io.head, io.rowstat, 1 if self.masked else 0, *io.d_out, *io.d_values, *io.d_head,
                                _lib.ptr(grads.d_source), *_lib.saved_out_args(grads.out), *(_lib.ptr(t) for t in rev), _lib.ptr(dv_ws), *io.tail)
        _lib.check(rc, "pit_distlist_bwd")


@torch.compiler.disable
def posatt_list_apply(values: torch.Tensor, lmda: torch.Tensor, plan: ListPlan, n_head: int, concat: bool = False,
                      head_is_scale: bool = False, sqd: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``posatt_dist_apply`` on candidate lists: out[b,n,h*D+d] = sum_t P[n,t] * values[b,idx[n,t],d] over the kept slots of row
    n (the kept set and the weights of pit.py:48-57 on the matrix that holds the listed distances and a masked value everywhere
    else); ``concat`` prepends the inputs (pit.py:44).  ``sqd``: the caller's own tensor (the one ``plan`` was built from); when
    grad mode is on and it requires grad it becomes an input of the node and receives d loss / d sqd in its shape, so autograd
    carries the gradient on to whatever formed the listed distances.  fp32 math mode only; head-scale routes as in ``posatt_apply``."""
    return _posatt_supplied_apply(values, lmda, plan, n_head, concat, head_is_scale, sqd)


# ---- one-launch MLP chains of the bf16 math mode (csrc/pit_chain.hip): hid 128 / 256 on a few thousand rows ----------------------
# The chains read their weights as bf16: copies are kept per weight tensor and re-formed when the weight changed (version counter /
# parameters_changed() epoch) - all requested copies in ONE launch.  Inside a stream capture nothing can be known about the
# weights at replay time (an optimizer between replays, or inside the graph): the cast is then always part of the graph, once per
# forward pass (pit.processor requests every block's weights at its entry: prepare_chain_weights).
CHAIN_MLP = os.environ.get("PIT_CHAIN_MLP", "1") != "0"


def chain_mlp_supported(rows: int, n0: int, n1: int, n2: int, out_gelu: bool) -> bool:
    return bool(CHAIN_MLP and out_gelu and get_math_mode() == "bf16"
                and _lib.lib().pit_mlp_chain_supported(int(rows), int(n0), int(n1), int(n2)))


def bf16_weights(tensors, new_pass: bool = False):
    """bf16 copies (RNE) of contiguous fp32 weight tensors.  The copy lives ON the tensor object it was made from (``_pit_bf16``:
    buffer, version counter, parameters_changed() epoch, address) - a key built from the address alone would hand a freed
    weight's copy to whatever tensor the allocator puts there next.  See the section comment for the capture rule."""
    cap = _capturing()
    if new_pass:
        _STEP.cap_fresh = set()
    fresh = getattr(_STEP, "cap_fresh", None) if cap else None
    out, need = [], []
    for t in tensors:
        ent = getattr(t, "_pit_bf16", None)
        if ent is None or ent[0].shape != t.shape or ent[0].device != t.device:
            ent = [torch.empty(t.shape, device=t.device, dtype=torch.bfloat16), -1, -1, 0]
            t._pit_bf16 = ent
        if cap:
            _pin(ent[0], t)
            stale = fresh is None or id(t) not in fresh
        else:
            stale = ent[1] != t._version or ent[2] != _PARAM_EPOCH[0] or ent[3] != t.data_ptr()
        if stale:
            need.append((t, ent))
        out.append(ent[0])
    if need:
        n = len(need)
        src = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _e in need])
        dst = (ctypes.c_void_p * n)(*[e[0].data_ptr() for _t, e in need])
        cnt = (ctypes.c_long * n)(*[t.numel() for t, _e in need])
        rc = _lib.lib().pit_cast_bf16_multi(n, src, dst, cnt, _lib.stream_ptr())
        _lib.check(rc, "pit_cast_bf16_multi")
        for t, ent in need:
            if cap:                       # recorded, not executed: the copy in memory is NOT this version
                ent[1] = ent[2] = -1
                if fresh is None:
                    fresh = _STEP.cap_fresh = set()
                fresh.add(id(t))
            else:
                ent[1], ent[2], ent[3] = t._version, _PARAM_EPOCH[0], t.data_ptr()
    return out


def _chain_weight_ok(w) -> bool:
    return torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.data_ptr() % 16 == 0 \
        and w.numel() % 4 == 0


def prepare_chain_weights(mlps, rows: int) -> None:
    """pit.processor's entry: the bf16 copies of every block MLP's weights that will take the chain launches, in one launch."""
    ws = []
    for w1, w2 in mlps:
        n1, n0 = w1.shape
        if w2.shape == (n1, n1) and chain_mlp_supported(rows, n0, n1, n1, True) and _chain_weight_ok(w1) and _chain_weight_ok(w2):
            ws += [w1, w2]
    if ws:
        bf16_weights(ws[:32], new_pass=True)


class _Mlp(torch.autograd.Function):
    """kaiming_mlp forward/backward, optionally with the trailing gelu of pit.py:111,121."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, out_gelu: bool, concat_heads: int = 0, satt_link=None, y16_slot=None, after_dense_att: bool = False,
                ordered: bool = False):
        _need_gpu(w1, b1, w2, b2)
        _need_gpu_bf16_ok(x)
        shape = x.shape
        n0 = shape[-1]
        n1, n2 = w1.shape[0], w2.shape[0]
        x16 = x.dtype == torch.bfloat16
        if x16 and (out_gelu or concat_heads > 0 or not mlp_bf16_io_supported(x.numel() // n0, n0, n1, n2)):
            x, x16 = x.float(), False              # (a bf16-stored input this shape's kernels do not read: widen once)
        x2 = x.reshape(-1, n0)
        if x2.stride(1) != 1 or x2.stride(0) < n0:
            x2 = x2.contiguous()
        rows = x2.shape[0]
        if w1.shape[1] != n0 or w2.shape[1] != n1:
            raise RuntimeError(f"mlp shapes do not chain: x[...,{n0}], w1{tuple(w1.shape)}, w2{tuple(w2.shape)}")
        w1c, b1c, w2c, b2c = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        dev = x.device
        save_dt = torch.bfloat16 if x16 else torch.float32      # decoder tail in bf16 storage: Z1 / H saved as bf16 too
        z1 = torch.empty((rows, n1), device=dev, dtype=save_dt)
        h = torch.empty((rows, n1), device=dev, dtype=save_dt)
        z2 = torch.empty((rows, n2), device=dev, dtype=torch.float32) if out_gelu else None
        buf = None
        if concat_heads > 0:             # y goes straight into columns [0, n2) of the next self-attention's concat buffer
            buf = torch.empty((rows, (1 + concat_heads) * n2), device=dev, dtype=torch.float32)
            y = buf[:, :n2]
        else:
            y = torch.empty((rows, n2), device=dev, dtype=torch.float32)
        ctx.math = _math_code() | ((IO_X_BF16 | IO_SAVE_BF16 | IO_DX_BF16) if x16 else 0)
        ctx.x16 = x16
        ctx.chain = None
        # ragged batches: the weight gradients are summed in a fixed order (pit_mlp_bwd_params_ordered) - fp32 tensors, the plain kernels
        # (2: the reproducible mode's pit_mlp_bwd_params_ordered_mfma)
        ctx.ordered = (2 if ordered == 2 else int(bool(ordered))) if not x16 else 0
        if not x16 and not ctx.ordered and chain_mlp_supported(rows, n0, n1, n2, out_gelu) and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0 \
                and _chain_weight_ok(w1) and _chain_weight_ok(w2):
            # bf16 mode, hid 128 / 256, a few thousand rows: GEMM1 + gelu + GEMM2 + gelu in ONE launch (csrc/pit_chain.hip)
            w1b, w2b = bf16_weights([w1, w2])
            # (feeding a self-attention layer: bf16(y) beside y, so that pit_satt_fwd needs no prep launch)
            y16 = torch.empty((rows, n2), device=dev, dtype=torch.bfloat16) if (y16_slot is not None and buf is not None and SATT_FUSE_PREP) else None
            rc = _lib.lib().pit_mlp_chain_fwd(x2.data_ptr(), x2.stride(0), rows, n0, n1, w1b.data_ptr(), b1c.data_ptr(),
                                              w2b.data_ptr(), b2c.data_ptr(), z1.data_ptr(), h.data_ptr(), z2.data_ptr(),
                                              y.data_ptr(), y.stride(0), _lib.ptr(y16), _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_chain_fwd")
            ctx.chain = (w1b, w2b)
            if y16 is not None:
                y16_slot.append(y16)
        else:
            rc = _lib.lib().pit_mlp_fwd(x2.data_ptr(), x2.stride(0), rows, n0, n1, n2, w1c.data_ptr(), b1c.data_ptr(),
                                        w2c.data_ptr(), b2c.data_ptr(), 1 if out_gelu else 0, z1.data_ptr(),
                                        h.data_ptr(), _lib.ptr(z2), y.data_ptr(), y.stride(0), ctx.math & ~IO_DX_BF16,
                                        _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_fwd")
        ctx.out_gelu, ctx.dims, ctx.in_shape = out_gelu, (rows, n0, n1, n2), shape
        ctx.satt_link = satt_link if ctx.chain is not None else None
        ctx.after_dense_att = bool(after_dense_att)
        ctx.params = (w1, b1, w2, b2)
        ctx.save_for_backward(x2, w1c, w2c, z1, h, z2 if out_gelu else z1)
        out = y.reshape(*shape[:-1], n2)             # (a view: constant row stride)
        if buf is None:
            return out
        buf = buf.reshape(*shape[:-1], (1 + concat_heads) * n2)
        ctx.mark_non_differentiable(buf)
        ctx.set_materialize_grads(False)             # no zero-filled "gradient" tensor for the buffer output
        return out, buf

    @staticmethod
    def backward(ctx, d_y, _d_buf=None):
        x2, w1, w2, z1, h, z2 = ctx.saved_tensors
        rows, n0, n1, n2 = ctx.dims
        if d_y is None:                              # (only with set_materialize_grads(False): output unused)
            d_y = torch.zeros((rows, n2), device=x2.device, dtype=torch.float32)
        dev = x2.device
        d_y2 = d_y.reshape(rows, n2)
        if d_y2.stride(1) != 1 or d_y2.stride(0) < n2:
            d_y2 = d_y2.contiguous()
        need_x = ctx.needs_input_grad[0]
        d_x = torch.empty((rows, n0), device=dev, dtype=torch.bfloat16 if ctx.x16 else torch.float32) if need_x else None
        # (fresh="empty": gradients returned to autograd are overwritten - accumulate = 0 - by the calls below; every postponed job
        # adds into the parameters' own .grad)
        grads, inplace = _mlp_grad_slots(ctx.params, ((n1, n0), (n1,), (n2, n1), (n2,)), ctx.needs_input_grad[1:5], dev, fresh="empty")
        d_w1, d_b1, d_w2, d_b2 = grads
        scratch = torch.empty((rows * (n1 + n2),), device=dev, dtype=torch.float32)
        L = _lib.lib()
        z2p = z2.data_ptr() if ctx.out_gelu else 0
        og = 1 if ctx.out_gelu else 0

        def postpone(math):                          # the weight-gradient reductions, handed to a later launch of the pass
            _dw_defer(*_params_job(x2, h, d_y2, scratch, grads, ctx.dims, og, math), dev)
        if ctx.ordered:
            # the data path, then both weight-gradient reductions slab by slab in a fixed order: the same bits on every run
            rc = L.pit_mlp_bwd_data(rows, n0, n1, n2, w1.data_ptr(), w2.data_ptr(), z1.data_ptr(), z2p, og,
                                    d_y2.data_ptr(), d_y2.stride(0), _lib.ptr(d_x), n0, scratch.data_ptr(),
                                    MATH_MODES["fp32"], _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_bwd_data")
            entry = "pit_mlp_bwd_params_ordered_mfma" if ctx.ordered == 2 else "pit_mlp_bwd_params_ordered"
            work = torch.empty((int(getattr(L, entry + "_workspace")(rows, n0, n1, n2)) // 4,), device=dev, dtype=torch.float32)
            rc = getattr(L, entry)(x2.data_ptr(), x2.stride(0), rows, n0, n1, n2, h.data_ptr(), og, d_y2.data_ptr(),
                                   d_y2.stride(0), d_w1.data_ptr(), d_b1.data_ptr(), d_w2.data_ptr(), d_b2.data_ptr(),
                                   1 if inplace else 0, scratch.data_ptr(), work.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, entry)
        elif ctx.chain is not None and d_y2.stride(0) % 4 == 0 and d_y2.data_ptr() % 16 == 0:
            # the data path (dZ2, dZ1, d_x) in ONE launch on the forward's bf16 weight copies, then both weight-gradient reductions
            w1b, w2b = ctx.chain
            # x is a self-attention layer's concat buffer (csrc/pit_satt.hip): its backward's G16 = bf16(d_x_h / rowsum_h) is written here,
            # beside d_x - that layer then needs no prep launch (it checks that the d_out it receives IS this d_x, unchanged: _handoff_g16_ready)
            lk, g16 = ctx.satt_link, None
            if (lk is not None and SATT_FUSE_PREP and d_x is not None and lk.get("rowstat") is not None and lk["dim"] == n1
                    and (1 + lk["n_head"]) * n1 == n0 and lk["batch"] * lk["pts"] == rows):
                g16 = torch.empty((lk["batch"], lk["n_head"], lk["pts"], n1), device=dev, dtype=torch.bfloat16)
            rc = L.pit_mlp_chain_bwd(rows, n0, n1, w1b.data_ptr(), w2b.data_ptr(), z1.data_ptr(), z2p, d_y2.data_ptr(),
                                     d_y2.stride(0), _lib.ptr(d_x), n0, scratch.data_ptr(), _lib.ptr(g16),
                                     lk["rowstat"].data_ptr() if g16 is not None else None, lk["pts"] if g16 is not None else 0,
                                     lk["mesh_batch"] if g16 is not None else 0, _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_chain_bwd")
            if g16 is not None:
                lk["g16"], lk["dx_ptr"], lk["dx_version"] = g16, d_x.data_ptr(), d_x._version
            if lk is not None and inplace and SATT_DW_RIDER and lk.get("rowstat") is not None:
                # the weight-gradient reductions depend on this launch only: they ride in the attention layer's ONE backward launch
                # (pit_satt_bwd's rider) instead of standing between the two
                postpone(ctx.math)
            else:
                rc = L.pit_mlp_bwd_params(x2.data_ptr(), x2.stride(0), rows, n0, n1, n2, h.data_ptr(), og, d_y2.data_ptr(),
                                          d_y2.stride(0), d_w1.data_ptr(), d_b1.data_ptr(), d_w2.data_ptr(), d_b2.data_ptr(),
                                          1 if inplace else 0, scratch.data_ptr(), ctx.math, _lib.stream_ptr())
                _lib.check(rc, "pit_mlp_bwd_params")
        elif MLP_PARAMS_RIDER and inplace and _dw_deferrable(rows, n0, n1, n2, og, d_y2.stride(0)):
            # dZ2, dZ1 and d_x now; the weight-gradient reductions ride along with the next attention backward
            rc = L.pit_mlp_bwd_data(rows, n0, n1, n2, w1.data_ptr(), w2.data_ptr(), z1.data_ptr(), z2p, og,
                                    d_y2.data_ptr(), d_y2.stride(0), _lib.ptr(d_x), n0, scratch.data_ptr(),
                                    ctx.math, _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_bwd_data")
            # (the postponed reductions of a small-regime MLP contract in fp32 in every math mode, like its fused data-path
            # kernels: as LDS-staged fp32 tiles they ride in the block launches at a third of the cost of the register-direct
            # bf16 form - bf16 mode at batch 8 was 5 % slower than fp32 for this alone)
            postpone(0)
        elif (WIDE_DW_RIDER and inplace and ctx.after_dense_att and not ctx.x16 and rows >= 1024 and n1 >= 128 and n1 % 64 == 0
              and n2 % 64 == 0 and n0 % 64 == 0 and (not og or d_y2.stride(0) == n2)):
            # x is the output of a dense self-attention layer (pit.py:116-121): the same split in the large regime - the reductions
            # (gemm_rr_kernel: 20-44 us between this MLP's backward and the attention's, which does not depend on them) ride in the
            # attention layer's merged backward launch as tiles (pit_posatt_bwd's rider -> posatt_bwd_pair_wide_kernel); a layer
            # that takes other kernels runs them as the launch they were.  (hid 128 / 256: at hid 64 the fused call's data path is the
            # slab kernel of csrc/pit_mlp_slab.hip, which pit_mlp_bwd_data does not take - Darcy b=256 159 k -> 151 k samples/s)
            rc = L.pit_mlp_bwd_data(rows, n0, n1, n2, w1.data_ptr(), w2.data_ptr(), z1.data_ptr(), z2p, og,
                                    d_y2.data_ptr(), d_y2.stride(0), _lib.ptr(d_x), n0, scratch.data_ptr(),
                                    ctx.math, _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_bwd_data")
            postpone(ctx.math)
        else:
            # one call: dZ1, then dX and both weight-gradient reductions (merged into one launch when small)
            # (small regime: fp32 in every math mode, like the postponed form above - the two must agree)
            small = not ctx.x16 and _dw_deferrable(rows, n0, n1, n2, og, d_y2.stride(0))
            rc = L.pit_mlp_bwd(x2.data_ptr(), x2.stride(0), rows, n0, n1, n2, w1.data_ptr(), w2.data_ptr(),
                               z1.data_ptr(), h.data_ptr(), z2p, og, d_y2.data_ptr(), d_y2.stride(0),
                               _lib.ptr(d_x), n0, d_w1.data_ptr(), d_b1.data_ptr(), d_w2.data_ptr(), d_b2.data_ptr(),
                               1 if inplace else 0, scratch.data_ptr(), 0 if small else ctx.math, _lib.stream_ptr())
            _lib.check(rc, "pit_mlp_bwd")
        dx = d_x.reshape(ctx.in_shape) if need_x else None
        # (forward's inputs: x, then w1, b1, w2, b2, then out_gelu, concat_heads, satt_link, y16_slot, after_dense_att, ordered)
        return (dx,) + ((None,) * 4 if inplace else tuple(grads)) + (None,) * 6


@torch.compiler.disable
def mlp_apply(x, w1, b1, w2, b2, out_gelu: bool = False, concat_heads: int = 0, ordered: bool = False) -> torch.Tensor:
    """kaiming_mlp forward (pit.py:21-26) (+ trailing gelu).  ``concat_heads=H`` (the result feeds a
    self-attention layer with H heads: pit.py:116-121) makes the kernels write the result directly into the
    first columns of that layer's (b, L, (1+H)*n2) concat buffer; the returned tensor is that strided view and
    carries the buffer (``_pit_concat``), so the attention kernel skips copying its inputs (pit.py:44).
    ``ordered`` (ragged batches, fp32 mode): the backward sums the weight gradients in a fixed order (pit_mlp_bwd_params_ordered)."""
    if not ordered and reproducible_wanted():        # (ordered: the ragged path keeps its own kernel, whose bits its tests pin)
        # reproducible mode: the data path, then pit_mlp_bwd_params_ordered_mfma; no rider, no hand-off (ordered = 2)
        if concat_heads <= 0 or x.dim() != 3:
            return _Mlp.apply(x, w1, b1, w2, b2, out_gelu, 0, None, None, False, 2)
        y, buf = _Mlp.apply(x, w1, b1, w2, b2, out_gelu, int(concat_heads), None, None, False, 2)
        y._pit_concat = buf
        return y
    if ordered:
        if get_math_mode() != "fp32":
            raise NotImplementedError("ordered weight gradients run in the fp32 math mode only")
        return _Mlp.apply(x, w1, b1, w2, b2, out_gelu, 0, None, None, False, True)
    link = getattr(x, "_pit_satt", None)         # x is the output of a dense self-attention layer on csrc/pit_satt.hip
    dense = bool(getattr(x, "_pit_dense_att", False))      # ... or of one on the fp32-era kernels (posatt_apply)
    if concat_heads <= 0 or x.dim() != 3:
        return _Mlp.apply(x, w1, b1, w2, b2, out_gelu, 0, link, None, dense)
    y16_slot = []
    y, buf = _Mlp.apply(x, w1, b1, w2, b2, out_gelu, int(concat_heads), link, y16_slot, dense)
    y._pit_concat = buf
    if y16_slot:
        y._pit_x16, y._pit_x16_version = y16_slot[0], y._version
    return y


# ---------------------------------------------------------------------------------------------------------------
# Fused processor (pit.py:114-122 on batch-free meshes, small regime): csrc/pit_block.hip
BLOCK_FUSION = os.environ.get("PIT_BLOCK_FUSION", "1") != "0"
BLOCK_MAX_LAYERS = 16              # MAX_LAYERS of csrc/pit_block_dev.h: blocks whose weights one pit_block_weights launch forms


def block_fusion_supported(n_pts: int, n_head: int, dim: int, batch: int, space_dim: int = 3) -> bool:
    """space_dim > 3: the per-layer kernels (the fused launches take at most three coordinates)."""
    return BLOCK_FUSION and space_dim <= 3 and bool(_lib.lib().pit_block_supported(int(n_pts), int(n_head), int(dim), int(batch)))


# Round 4: large-regime self-attention of batch-free models on PRECOMPUTED weights (pit_posatt_pre_fwd / _bwd): the weights
# of all processor blocks from ONE pit_block_weights launch per step, the attention launches read them instead of re-forming
# exp(-c m) in every workgroup.  PIT_PRE_WEIGHTS=0: the recompute-from-coordinates kernels.
PRE_WEIGHTS = os.environ.get("PIT_PRE_WEIGHTS", "1") != "0"


def pre_weights_supported(n_pts: int, n_head: int, dim: int, batch: int, space_dim: int = 3) -> bool:
    """space_dim > 3: the per-layer kernels (pit_block_weights takes at most three coordinates)."""
    return PRE_WEIGHTS and space_dim <= 3 and bool(_lib.lib().pit_posatt_pre_supported(int(n_pts), int(n_head), int(dim), int(batch)))


def block_weights(plan: "MeshPlan", lmdas, n_head: int, need_q: bool = True):
    """Softmax weights of len(lmdas) unmasked self-attention layers on one batch-free mesh (pit_block_weights, in launches of
    at most BLOCK_MAX_LAYERS layers): (E, Q or None, inv, rowstat, scale), each with a leading layer axis.  Route 'host':
    the host-evaluated head scales are what the kernel gets."""
    n, L, dev = len(lmdas), plan.n_in, plan.mesh_in.device
    scales = [host_head_scale(p) for p in lmdas] if get_head_scale_route() == "host" else None
    heads = [t.detach().reshape(-1).contiguous() for t in lmdas]
    kheads = scales if scales is not None else heads
    E = torch.empty((n, n_head, L, L), device=dev, dtype=torch.float32)
    Q = torch.empty((n, n_head, L, L), device=dev, dtype=torch.float32) if need_q else None
    inv = torch.empty((n, n_head, L), device=dev, dtype=torch.float32)
    rowstat = torch.empty((n, n_head, L, 4), device=dev, dtype=torch.float32)
    scale = torch.empty((n, n_head), device=dev, dtype=torch.float32)
    for l0 in range(0, n, BLOCK_MAX_LAYERS):
        m = min(BLOCK_MAX_LAYERS, n - l0)
        hp = (ctypes.c_void_p * m)(*[t.data_ptr() for t in kheads[l0:l0 + m]])
        rc = _lib.lib().pit_block_weights(plan.mesh_in.data_ptr(), L, plan.sdim, plan.metric_id, plan.period, m, hp,
                                          1 if scales is not None else 0, n_head, E[l0].data_ptr(),
                                          Q[l0].data_ptr() if Q is not None else None, inv[l0].data_ptr(),
                                          rowstat[l0].data_ptr(), scale[l0].data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_block_weights")
    return E, Q, inv, rowstat, scale, heads


class _PosAttPre(torch.autograd.Function):
    """posatt.forward (pit.py:37-44) of a batch-free self-attention layer with locality 1.0 on precomputed weights:
    out = cat((values, conv), -1).  Tensor inputs: values, lmda (flat); e / q / rowstat / scale are this layer's slices of
    block_weights' outputs (functions of the mesh and lmda: d(lmda) is delivered through the saved q)."""

    @staticmethod
    def forward(ctx, values, head, e, q, rowstat, scale, n_head: int, head_param, out_slot):
        _need_gpu(values, head)
        b, L, D = values.shape
        W = (1 + n_head) * D
        if values.stride(2) != 1:
            values = values.contiguous()
        given = out_slot[0] if out_slot else None
        out = given if given is not None else torch.empty((b, L, W), device=values.device, dtype=torch.float32)
        ctx.math = _math_code()
        rc = _lib.lib().pit_posatt_pre_fwd(e.data_ptr(), rowstat.data_ptr(), L, n_head, D, b, values.data_ptr(), values.stride(1),
                                           values.stride(0), out.data_ptr(), W, L * W, D, 0 if given is not None else 1,
                                           ctx.math, _lib.stream_ptr())
        _lib.check(rc, "pit_posatt_pre_fwd")
        ctx.n_head, ctx.head_param = n_head, head_param
        ctx.save_for_backward(values, head, e, q, rowstat, scale)
        return out

    @staticmethod
    def backward(ctx, d_out):
        values, head, e, q, rowstat, scale = ctx.saved_tensors
        n_head = ctx.n_head
        b, L, D = values.shape
        d_out = _row_view(d_out)
        if d_out.dtype != torch.float32:
            d_out = d_out.float()
        need_v, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dev = values.device
        d_values = torch.empty((b, L, D), device=dev, dtype=torch.float32)
        if need_h and q is None:
            raise RuntimeError("d(lmda) needs the d(scale) weights: block_weights(..., need_q=True)")
        # (head_is_scale=False: `head` is always lmda here - block_weights hands the kernels a host-evaluated scale beside it, never
        # in its place - so the finishing kernel applies the chain rule through lmda on either route)
        hg = _HeadGrad(ctx.head_param, need_h, n_head, dev, head_is_scale=False)
        _dw_run_pending(dev)                        # (a postponed MLP job: these launches carry nothing)
        rc = _lib.lib().pit_posatt_pre_bwd(e.data_ptr(), _lib.ptr(q), rowstat.data_ptr(), L, n_head, D, b, values.data_ptr(),
                                           values.stride(1), values.stride(0), d_out.data_ptr(), d_out.stride(1), d_out.stride(0),
                                           D, d_values.data_ptr(), D, L * D, 1, _lib.ptr(hg.work), ctx.math, _lib.stream_ptr())
        _lib.check(rc, "pit_posatt_pre_bwd")
        # (forward's inputs: values, head, then e, q, rowstat, scale, n_head, head_param, out_slot)
        return ((d_values if need_v else None), hg.finish(head, scale)) + (None,) * 7


@torch.compiler.disable
def posatt_pre_apply(values: torch.Tensor, lmda: torch.Tensor, weights, layer: int, n_head: int) -> torch.Tensor:
    """cat((values, conv), -1) of processor block ``layer`` from ``weights`` = block_weights(...)."""
    E, Q, _inv, rowstat, scale, _heads = weights
    out_buf = _concat_buffer_of(values, values.shape[1], n_head)
    slot = [out_buf] if out_buf is not None else None
    param = lmda if isinstance(lmda, torch.nn.Parameter) else None
    return _PosAttPre.apply(values, lmda.reshape(-1), E[layer], Q[layer] if Q is not None else None, rowstat[layer], scale[layer],
                            n_head, param, slot)


# The fused processor's softmax weights (pit_block_weights) depend on the latent mesh and the lmda's only - not on the data -
# so their launch need not sit in the step's chain between the encoder and the first block.  PIT_EARLY_WEIGHTS:
#   "rider" (default)  extra workgroups of the down-projection's launch form them (pit_posatt_fwd_job: one launch less in the
#                      chain); a down-projection that is not one of the small candidate-list launches gets them as a launch
#                      of their own right after it - the order of round 3, one call earlier.
#   (a side stream under the down-projection - a parallel branch of the step graph - was measured slower twice, rounds 3 and 4:
#   Darcy b=8 0.194 -> 0.222 ms/step; a straight chain of kernels is the fastest graph this runtime replays; removed in round 5)
#   "0"                formed by _Processor.forward itself (round 3).
EARLY_WEIGHTS = os.environ.get("PIT_EARLY_WEIGHTS", "rider")


class EarlyWeights:
    """Weights of all blocks (pit_block_weights) requested before the processor runs; join() before anything reads them."""
    __slots__ = ("key", "E", "Q", "inv", "rowstat", "scale", "job", "keep")

    def join(self) -> None:
        if getattr(_STEP, "fwd_job", None) is self:        # no attention launch took the job: a launch of its own, now
            _STEP.fwd_job = None
            j = self.job
            rc = _lib.lib().pit_block_weights(j.mesh, j.n_pts, j.space_dim, j.metric, j.period, j.n_layers, j.heads,
                                              j.head_is_scale, j.n_head, j.e, j.q, j.inv, j.rowstat, j.scale_out,
                                              _lib.stream_ptr())
            _lib.check(rc, "pit_block_weights")


def drop_forward_job(early) -> None:
    """Disarm ``early`` if no launch took it (pit.encoder's finally: a forward that raised leaves nothing pending on the thread)."""
    if early is not None and getattr(_STEP, "fwd_job", None) is early:
        _STEP.fwd_job = None
    _STEP.dec_job = None                         # (a decoder-weights request nobody carried: the decoder forms them itself)


def _weights_key(plan: MeshPlan, lmdas, scales, n_head: int):
    return (id(plan), n_head, _PARAM_EPOCH[0], scales is not None,
            tuple((p._version, p.data_ptr()) for p in lmdas), tuple(t.data_ptr() for t in scales) if scales is not None else None)


def _weights_buffers(plan: MeshPlan, n: int, n_head: int, need_q: bool):
    L, dev = plan.n_in, plan.mesh_in.device
    E = torch.empty((n, n_head, L, L), device=dev, dtype=torch.float32)
    # (Q, the d(scale) weights, is only read by the backward: not formed under no_grad / in eval)
    Q = torch.empty((n, n_head, L, L), device=dev, dtype=torch.float32) if need_q else None
    inv = torch.empty((n, n_head, L), device=dev, dtype=torch.float32)
    rowstat = torch.empty((n, n_head, L, 4), device=dev, dtype=torch.float32)
    scale = torch.empty((n, n_head), device=dev, dtype=torch.float32)
    return E, Q, inv, rowstat, scale


def _launch_block_weights(plan: MeshPlan, kheads, is_scale: bool, n_head: int, need_q: bool, stream_ptr):
    n = len(kheads)
    E, Q, inv, rowstat, scale = _weights_buffers(plan, n, n_head, need_q)
    hp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in kheads])
    rc = _lib.lib().pit_block_weights(plan.mesh_in.data_ptr(), plan.n_in, plan.sdim, plan.metric_id, plan.period, n, hp,
                                      1 if is_scale else 0, n_head, E.data_ptr(), _lib.ptr(Q), inv.data_ptr(),
                                      rowstat.data_ptr(), scale.data_ptr(), stream_ptr)
    _lib.check(rc, "pit_block_weights")
    return E, Q, inv, rowstat, scale


def early_block_weights(plan: MeshPlan, lmdas, n_head: int, need_q: bool):
    """Request pit_block_weights for processor_apply(x, plan, n_head, lmdas, ...) BEFORE the layer in front of the processor
    runs (modes: EARLY_WEIGHTS above).  The caller join()s the returned handle on the same stream before its function ends
    (nothing is left pending or unjoined) and hands it to processor_apply, which uses it when lmdas / scales are still the ones
    it was formed from."""
    if EARLY_WEIGHTS != "rider" or not plan.mesh_in.is_cuda:
        return None
    scales = [host_head_scale(p) for p in lmdas] if get_head_scale_route() == "host" else None
    heads = [t.detach().reshape(-1).contiguous() for t in lmdas]
    kheads = scales if scales is not None else heads
    ew = EarlyWeights()
    ew.key = _weights_key(plan, lmdas, scales, n_head)
    ew.job = ew.keep = None
    n = len(kheads)
    ew.E, ew.Q, ew.inv, ew.rowstat, ew.scale = _weights_buffers(plan, n, n_head, need_q)
    hp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in kheads])
    ew.keep = (hp, kheads, plan)
    ew.job = _lib.BlockWeightsJob(plan.mesh_in.data_ptr(), plan.n_in, plan.sdim, plan.metric_id, plan.period, n,
                                  ctypes.cast(hp, ctypes.c_void_p), 1 if scales is not None else 0, n_head,
                                  ew.E.data_ptr(), _lib.ptr(ew.Q), ew.inv.data_ptr(), ew.rowstat.data_ptr(), ew.scale.data_ptr())
    _STEP.fwd_job = ew                       # the next attention forward of this thread carries it (_PosAtt.forward)
    return ew


class _Processor(torch.autograd.Function):
    """n_blocks x [posatt.forward -> kaiming_mlp -> gelu] (pit.py:114-122) on one batch-free latent mesh as ONE
    autograd node: the softmax weights of all blocks come from one launch (pit_block_weights: they depend on the mesh
    and the lmda's only), every block's forward is one launch (pit_block_fwd) and its backward chain one launch
    (pit_block_bwd: d(values) of block i + the data path of block i-1's MLP backward, with block i's d(scale) and its
    MLP's weight-gradient reductions riding along).  Tensor inputs: x, lmda_0..n-1, then (w1, b1, w2, b2) per block."""

    @staticmethod
    def forward(ctx, x, plan: MeshPlan, n_head: int, scales, params, early, *tensors):
        n = len(tensors) // 5
        lmdas, mlps = tensors[:n], [tensors[n + 4 * i:n + 4 * i + 4] for i in range(n)]
        _need_gpu(x, *tensors)
        b, L, D = x.shape
        H, W, rows = n_head, (1 + n_head) * D, b * L
        dev = x.device
        L_ = _lib.lib()
        # the fused blocks contract in exact fp32 in EVERY math mode: the small regime is latency-bound (an MFMA form 16x as fast
        # changes nothing) and fp32 products are inside any bf16 tolerance - so the bf16 mode never loses to fp32 at the scripts'
        # batch 8 (round 3: 31.8 k vs 40.1 k samples/s because bf16 mode fell back to one launch per layer)
        ctx.math = 0
        heads = [t.detach().reshape(-1).contiguous() for t in lmdas]
        kheads = list(scales) if scales is not None else heads         # route 'host': the host-evaluated c is what the kernels get
        need_q = any(ctx.needs_input_grad)
        if early is not None and early.key == _weights_key(plan, params[0], scales, H) and (early.Q is not None or not need_q):
            E, Q, inv, rowstat, scale = early.E, early.Q, early.inv, early.rowstat, early.scale   # (formed under the encoder)
        else:
            E, Q, inv, rowstat, scale = _launch_block_weights(plan, kheads, scales is not None, H, need_q, _lib.stream_ptr())
        buf0 = _concat_buffer_of(x, L, H)
        if buf0 is None:                       # the producer did not write into a concat buffer: one copy
            buf0 = torch.empty((b, L, W), device=dev, dtype=torch.float32)
            buf0[:, :, :D].copy_(x.detach())
        else:
            buf0 = buf0.detach()
        bufs = [buf0] + [torch.empty((b, L, W), device=dev, dtype=torch.float32) for _ in range(n - 1)]
        out = torch.empty((b, L, D), device=dev, dtype=torch.float32)
        z1 = torch.empty((n, rows, D), device=dev, dtype=torch.float32)
        hh = torch.empty((n, rows, D), device=dev, dtype=torch.float32)
        z2 = torch.empty((n, rows, D), device=dev, dtype=torch.float32)
        wts = [tuple(t.detach().contiguous() for t in m) for m in mlps]
        for i in range(n):
            w1, b1, w2, b2 = wts[i]
            if tuple(w1.shape) != (D, W) or tuple(w2.shape) != (D, D):
                raise RuntimeError(f"fused processor: block {i} MLP is {tuple(w1.shape)} / {tuple(w2.shape)}, expected "
                                   f"({D}, {W}) / ({D}, {D})")
        for i in range(n):
            y, ldy = (bufs[i + 1], W) if i + 1 < n else (out, D)
            w1, b1, w2, b2 = wts[i]
            rc = L_.pit_block_fwd(E[i].data_ptr(), inv[i].data_ptr(), L, H, D, b, bufs[i].data_ptr(), w1.data_ptr(),
                                  b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), 1, z1[i].data_ptr(), hh[i].data_ptr(),
                                  z2[i].data_ptr(), y.data_ptr(), ldy, ctx.math, _lib.stream_ptr())
            _lib.check(rc, "pit_block_fwd")
        ctx.n, ctx.H, ctx.dims, ctx.plan = n, H, (b, L, D), plan
        ctx.params = params                    # (lmda parameters, (w1, b1, w2, b2) parameters) for the in-place gradient slots
        ctx.hook = _processor_hook()           # the caller's per-thread step state
        ctx.repro = get_reproducible()         # (read on the calling thread: the backward runs on autograd's)
        ctx.keep = (bufs, wts, heads, E, Q, inv, scale, z1, hh, z2)
        return out

    @staticmethod
    def backward(ctx, d_out):
        n, H = ctx.n, ctx.H
        b, L, D = ctx.dims
        W, rows = (1 + H) * D, b * L
        bufs, wts, heads, E, Q, inv, scale, z1, hh, z2 = ctx.keep
        lm_params, mlp_params = ctx.params
        dev = d_out.device
        L_ = _lib.lib()
        d_out = d_out.contiguous()
        dxc = [torch.empty((b, L, W), device=dev, dtype=torch.float32) for _ in range(n)]
        scratch = [torch.empty((rows * 2 * D,), device=dev, dtype=torch.float32) for _ in range(n)]
        dx = torch.empty((b, L, D), device=dev, dtype=torch.float32)
        # gradient destinations: the parameters' own .grad slots (in place, nothing returned) or fresh tensors
        # (needs: not consulted here - a block whose four parameters all opted in accumulates in place)
        w_grads = [_mlp_grad_slots(mlp_params[i], [t.shape for t in wts[i]], (True,) * 4, dev) for i in range(n)]
        # (head_is_scale=False: `heads` are the lmda's themselves on either route; d(lmda) of every block is always formed)
        hgs = [_HeadGrad(p if isinstance(p, torch.nn.Parameter) else None, True, H, dev, head_is_scale=False) for p in lm_params]
        # a large job the pass has postponed (the decoder MLP's weight gradients): one row slice per block launch
        extra = _dw_take(dev)
        slices = []
        sliceable = False
        if extra is not None:
            st = extra[0]
            sliceable = bool(not st.out_gelu and st.accumulate and (st.math_mode & 0xff) == 0)
        # which launch carries what (rider_tail_schedule): the last k launches give their jobs to the pass's finishing launch
        k_tail, n_slices, plan = rider_tail_schedule(n, RIDER_TAIL_BLOCKS, None if ctx.hook is None else ctx.hook[1], ctx.repro,
                                                     all(inplace for _, inplace in w_grads), all(h.defer for h in hgs), sliceable,
                                                     2 * 8 * ((b + 7) // 8) * (L // 16) <= _cu_count(dev))
        if extra is not None:
            if sliceable:
                # a two-bucket step reduces the postponed job's gradients right after block `complete_by`: every
                # slice must ride in a launch up to that one
                slices = _dw_slices(extra, n_slices)
            else:
                _dw_run(extra)
        stream = torch.cuda.current_stream(dev)
        # top of the chain: the last block's MLP backward (data path) from d_out
        w1, _, w2, _ = wts[n - 1]
        rc = L_.pit_mlp_bwd_data(rows, W, D, D, w1.data_ptr(), w2.data_ptr(), z1[n - 1].data_ptr(), z2[n - 1].data_ptr(), 1,
                                 d_out.data_ptr(), D, dxc[n - 1].data_ptr(), W, scratch[n - 1].data_ptr(), ctx.math,
                                 _lib.stream_ptr())
        _lib.check(rc, "pit_mlp_bwd_data")
        for i in range(n - 1, -1, -1):
            job = _params_job(bufs[i], hh[i], scratch[i], scratch[i], w_grads[i][0], (rows, W, D, D), 1, ctx.math, ld_dy=D)[0]
            if i > 0:
                pw1, _, pw2, _ = wts[i - 1]
                prev = (pw1.data_ptr(), pw2.data_ptr(), z1[i - 1].data_ptr(), z2[i - 1].data_ptr(), 1, W,
                        dxc[i - 1].data_ptr(), W, scratch[i - 1].data_ptr(), None, 0)
            else:
                prev = (None, None, None, None, 0, 0, None, 0, None, dx.data_ptr(), D)
            k = n - 1 - i                              # launch order
            own_to, slice_to = plan[k]
            job1 = ctypes.cast(ctypes.pointer(job), ctypes.c_void_p) if own_to == "launch" else None
            job2 = ctypes.cast(ctypes.pointer(slices[k]), ctypes.c_void_p) if k < len(slices) and slice_to == "launch" else None
            rc = L_.pit_block_bwd(E[i].data_ptr(), inv[i].data_ptr(), Q[i].data_ptr(), L, H, D, b, dxc[i].data_ptr(),
                                  bufs[i].data_ptr(), hgs[i].work.data_ptr(), *prev, job1, job2, ctx.math,
                                  _lib.stream_ptr())
            _lib.check(rc, "pit_block_bwd")
            if own_to == "tail":                       # (after the launch: its chain wrote the dZ1 | dZ2 the job reads)
                _tail_defer([(job, (bufs[i], hh[i], scratch[i]) + tuple(w_grads[i][0]), stream)])
            if k < len(slices) and slice_to == "tail":
                _tail_defer([(slices[k], extra[1], stream)])
            if ctx.hook is not None:
                ctx.hook[0](i)                              # (block i's weight gradients are now enqueued)
        # d(lmda): deferred layers are finished by the pass's one finishing launch; the others here, in one launch
        d_heads = _HeadGrad.finish_all([(hgs[i], heads[i], scale[i]) for i in range(n)])
        # (forward's inputs: x, then plan, n_head, scales, params, early - then the n lmda's - then (w1, b1, w2, b2) per block)
        grads = (dx,) + (None,) * 5 + tuple(d_heads)
        for g, inplace in w_grads:
            grads += (None,) * 4 if inplace else tuple(g)
        return grads


# engine.TrainStep(all_reduce_buckets=2) sets step_state(processor_hook=(callback, complete_by)): the callback is called
# with the block index after each block's backward launch; everything the pass postponed before the processor (the
# decoder MLP's weight gradients) must be enqueued by the launch of block `complete_by`, after which the step all-reduces
# those gradients on its second stream.  Per thread, carried by the autograd node (see _STEP).


@torch.compiler.disable
def processor_apply(x: torch.Tensor, plan: MeshPlan, n_head: int, lmdas, mlps, early=None) -> torch.Tensor:
    """The whole processor (pit.py:114-122) on a batch-free mesh through the fused block kernels.  ``lmdas``: the
    blocks' lmda parameters; ``mlps``: per block (w1, b1, w2, b2); ``early``: early_block_weights(...) of the same plan and
    lmdas, already joined.  The caller checked block_fusion_supported()."""
    scales = None
    if get_head_scale_route() == "host":
        scales = [host_head_scale(p) for p in lmdas]
    flat = [p.reshape(-1) for p in lmdas] + [t for m in mlps for t in m]
    return _Processor.apply(x, plan, n_head, scales, (tuple(lmdas), tuple(tuple(m) for m in mlps)), early, *flat)


# ---------------------------------------------------------------------------------------------------------------
# Round 5: the encoder side (pit.py:108-112) and the decoder side (pit.py:124-127) of a small-regime model on batch-free
# meshes as ONE launch per direction each (csrc/pit_edge.hip), on the static slab plan of the mesh pair.
EDGE_FUSION = os.environ.get("PIT_EDGE_FUSION", "1") != "0"


def edge_fusion_supported(plan: MeshPlan, n_head: int, dim: int, batch: int, needs_union: bool) -> bool:
    """The fused encoder- / decoder-side launch covers this layer: a masked cross-attention on a batch-free mesh pair with
    complete candidate lists (and, for the decoder, unions of at most 64 keys per 16-row slab), 1-2 heads, hidden width 32 / 64,
    in the latency regime."""
    if not EDGE_FUSION or plan.mesh_batch != 1 or plan.self_attn or not plan.masked or plan.nbr_idx is None or plan.sdim > 3:
        return False
    if needs_union and torch.are_deterministic_algorithms_enabled():     # (the decoder's d(values): fp32 atomic adds)
        return False
    if not _lib.lib().pit_edge_supported(int(n_head), int(dim), int(batch), int(plan.n_out)):
        return False
    sp = plan.slab_plan(patch=needs_union)          # (needs_union: the fused decoder, the one consumer of patch plans)
    return sp is not None and (not needs_union or sp[1] <= SLAB_UNION_MAX)


class LossSpec:
    """The RelLp loss a training step will apply to the model's prediction (engine.TrainStep sets it in step_state): the fused
    decoder forward accumulates the loss's partial sums in its epilogue, the decoder backward forms d(pred) from them - the step
    then has no loss launch.  ``true`` (b, npts, out_dim) contiguous, ``scale`` / ``shift`` (npts, out_dim) or None, p in {1, 2}."""
    __slots__ = ("true", "scale", "shift", "p", "out_dim", "seed", "partials", "pred", "token", "value")

    def __init__(self, true, scale, shift, out_dim: int, p: int, seed=None):
        b = true.size(0)
        self.true = true.reshape(b, -1, out_dim).contiguous()
        npts = self.true.shape[1]
        self.scale = scale.reshape(npts, out_dim).contiguous() if scale is not None else None
        self.shift = shift.reshape(npts, out_dim).contiguous() if shift is not None else None
        self.p, self.out_dim, self.seed = int(p), int(out_dim), seed
        self.partials = self.pred = self.token = self.value = None

    def fits(self, batch: int, npts: int, n2: int) -> bool:
        return self.p in (1, 2) and n2 == self.out_dim and tuple(self.true.shape) == (batch, npts, n2) and not self.true.requires_grad


class DecoderWeights:
    """The up-projection's softmax weights of one step (pit_decoder_weights): P / Q tiles per 16-row slab and the head scales c.
    They depend on (mesh pair, lmda) only: formed once per step - by extra workgroups of the encoder-side launch when pit.encoder
    could request them (early_decoder_weights), else by a launch of their own in front of the decoder launch."""
    __slots__ = ("key", "pw", "qw", "scale", "job", "keep", "w1f", "slab", "max_union")


def _dec_weights_key(plan: MeshPlan, lmda, scale_in, n_head: int, head_is_scale: bool, w1=None):
    return (id(plan), n_head, _PARAM_EPOCH[0], lmda._version, lmda.data_ptr(), bool(head_is_scale),
            scale_in.data_ptr() if scale_in is not None else None,
            (w1.data_ptr(), w1._version, tuple(w1.shape)) if w1 is not None else None)


def _new_decoder_weights(plan: MeshPlan, lmda, scale_in, n_head: int, head_is_scale: bool, need_q: bool, w1=None,
                         patch: bool = True) -> DecoderWeights:
    """``patch``: on MeshPlan.slab_plan(patch=True) - the fused decoder's plan (tiles of 16 slots when no patch holds more keys);
    False: on the consecutive plan (pit_union_att_*).  The launches that consume the tiles run on the plan they were formed
    on (``slab`` / ``max_union`` of the result)."""
    sp, max_union, _t, max_count = plan.slab_plan(patch)
    um = _lib.lib().pit_decoder_union_slots(ctypes.byref(sp), max_union)      # (16 | 32 | 48 | 64: the launches' own choice)
    dev = plan.mesh_out.device
    w = DecoderWeights()
    w.key = _dec_weights_key(plan, lmda, scale_in, n_head, head_is_scale, w1)
    w.slab, w.max_union = sp, max_union
    # the decoder MLP's W1 in MFMA-fragment order (pit_hip.h: w1f): formed with the tiles, once per step
    w1c = w1.detach() if (w1 is not None and w1.is_contiguous() and w1.dtype == torch.float32 and w1.dim() == 2
                          and w1.shape[0] % 16 == 0 and w1.shape[1] == n_head * w1.shape[0] and w1.data_ptr() % 16 == 0) else None
    w.w1f = torch.empty_like(w1c) if w1c is not None else None
    w.pw = torch.empty((sp.n_slabs, n_head, 16, um), device=dev, dtype=torch.float32)
    w.qw = torch.empty((sp.n_slabs, n_head, 16, um), device=dev, dtype=torch.float32) if need_q else None
    w.scale = torch.empty((n_head,), device=dev, dtype=torch.float32)
    head = scale_in if scale_in is not None else lmda.detach().reshape(-1).contiguous()
    w.keep = (head, plan, sp, w1c)
    w.job = _lib.DecoderWeightsJob(ctypes.cast(ctypes.pointer(sp), ctypes.c_void_p), head.data_ptr(),
                                   1 if (scale_in is not None or head_is_scale) else 0, n_head, max_union, max_count,
                                   w.pw.data_ptr(), _lib.ptr(w.qw), w.scale.data_ptr(),
                                   _lib.ptr(w1c), _lib.ptr(w.w1f), w1c.shape[0] if w1c is not None else 0)
    return w


def _launch_decoder_weights(w: DecoderWeights) -> None:
    j = w.job
    rc = _lib.lib().pit_decoder_weights(j.plan, j.head, j.head_is_scale, j.n_head, j.max_union, j.max_count, j.pw, j.qw,
                                        j.scale_out, j.w1, j.w1f, j.dim, _lib.stream_ptr())
    _lib.check(rc, "pit_decoder_weights")


def early_decoder_weights(plan: MeshPlan, lmda, n_head: int, need_q: bool, w1=None) -> None:
    """Request the decoder's weights BEFORE the encoder-side launch of the same forward (pit.encoder): encoder_apply carries the job
    in its launch; decoder_apply uses the result when plan / lmda / route are still the ones it was formed from.  A job no launch
    took is dropped (drop_forward_job) - the decoder then forms its weights itself."""
    scale_in = host_head_scale(lmda) if get_head_scale_route() == "host" else None
    _STEP.dec_job = _new_decoder_weights(plan, lmda, scale_in, n_head, False, need_q, w1)
    _STEP.dec_ready = None


class _Decoder(torch.autograd.Function):
    """pit.decoder (pit.py:124-127): posatt_cross_* (mesh_ltt -> mesh_out) followed by the thin-output kaiming_mlp `de`."""

    @staticmethod
    def forward(ctx, values, head, plan: MeshPlan, n_head: int, head_is_scale: bool, head_param, weights, params, loss, w1, b1, w2, b2):
        _need_gpu(values, head, w1, b1, w2, b2)
        values = _row_view(values)
        if values.stride(1) % 4 or values.stride(0) % 4 or values.data_ptr() % 16:
            values = values.contiguous()
        b, j, d = values.shape
        n2 = w2.shape[0]
        dev = values.device
        sp = weights.slab                      # (the plan the step's tiles were formed on)
        head = head.detach().reshape(-1).contiguous()
        w1c, b1c, w2c, b2c = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        rows = b * plan.n_out
        need = weights.qw is not None          # (decoder_apply asked for the d(scale) tiles exactly when a backward can follow)
        y = torch.empty((b, plan.n_out, n2), device=dev, dtype=torch.float32)
        x = z1 = h = dvals = None
        if need:
            x = torch.empty((rows, n_head * d), device=dev, dtype=torch.float32)
            z1 = torch.empty((rows, d), device=dev, dtype=torch.float32)
            h = torch.empty((rows, d), device=dev, dtype=torch.float32)
            dvals = torch.empty((b, j, d), device=dev, dtype=torch.float32)       # zeroed by the launch, added to by the backward
        lt = ls = lh = lpart = None
        lp = 0
        if loss is not None and need:
            lt, ls, lh, lp = loss.true, loss.scale, loss.shift, loss.p
            lpart = loss.partials = torch.empty((b, n2, sp.n_slabs, 2), device=dev, dtype=torch.float64)
            loss.value = torch.empty((), device=dev, dtype=torch.float32)
        # (the fragment-order copy of W1 belongs to the tensor the weights were formed from)
        w1f = weights.w1f if (weights.w1f is not None and weights.keep[3].data_ptr() == w1c.data_ptr()) else None
        rc = _lib.lib().pit_decoder_fwd(ctypes.byref(sp), values.data_ptr(), values.stride(1), values.stride(0), b, n_head, d,
                                        weights.pw.data_ptr(), w1c.data_ptr(), _lib.ptr(w1f), b1c.data_ptr(), w2c.data_ptr(),
                                        b2c.data_ptr(), n2, _lib.ptr(x), _lib.ptr(z1), _lib.ptr(h), y.data_ptr(),
                                        _lib.ptr(dvals), dvals.numel() if dvals is not None else 0,
                                        _lib.ptr(lt), _lib.ptr(ls), _lib.ptr(lh), lp, _lib.ptr(lpart), weights.max_union,
                                        _lib.stream_ptr())
        _lib.check(rc, "pit_decoder_fwd")
        ctx.plan, ctx.n_head, ctx.head_is_scale, ctx.head_param, ctx.params = plan, n_head, head_is_scale, head_param, params
        ctx.loss = loss if lpart is not None else None
        if ctx.loss is not None:
            loss.pred = y
        ctx.dvals_clean = True
        ctx.keep = (values, head, w1c, w2c, x, z1, h, weights, dvals)
        return y

    @staticmethod
    def backward(ctx, d_y):
        values, head, w1, w2, x, z1, h, weights, dvals = ctx.keep
        scale = weights.scale
        plan, n_head = ctx.plan, ctx.n_head
        b, j, d = values.shape
        n2, rows = w2.shape[0], b * plan.n_out
        dev = values.device
        sp = weights.slab
        loss = ctx.loss
        inside = loss is not None and loss.token is not None and d_y.data_ptr() == loss.token.data_ptr()
        if loss is not None and loss.token is not None and not inside:
            raise RuntimeError("the fused loss's gradient token reached pit.decoder's backward as a copy: the prediction must reach "
                               "the loss through views only (engine.TrainStep)")
        if not ctx.dvals_clean:                         # a second backward through the same node (retain_graph)
            dvals.zero_()
        ctx.dvals_clean = False
        dz1 = torch.empty((rows, d), device=dev, dtype=torch.float32)
        if inside:
            d_pred = torch.empty((rows, n2), device=dev, dtype=torch.float32)
            dyp, ld = None, n2
        else:
            d_pred = d_y.reshape(rows, n2)
            if d_pred.stride(1) != 1 or d_pred.stride(0) < n2:
                d_pred = d_pred.contiguous()
            dyp, ld = d_pred, d_pred.stride(0)
        hg = _HeadGrad(ctx.head_param, ctx.needs_input_grad[1], n_head, dev, ctx.head_is_scale)
        L = _lib.lib()
        rc = L.pit_decoder_bwd(ctypes.byref(sp), values.data_ptr(), values.stride(1), values.stride(0), b, n_head, d,
                               weights.pw.data_ptr(), weights.qw.data_ptr(), w1.data_ptr(), w2.data_ptr(), n2, z1.data_ptr(),
                               _lib.ptr(dyp), ld, dz1.data_ptr(), dvals.data_ptr(), dvals.stride(0), _lib.ptr(hg.work),
                               loss.pred.data_ptr() if inside else None, _lib.ptr(loss.true) if inside else None,
                               _lib.ptr(loss.scale) if inside else None, _lib.ptr(loss.shift) if inside else None,
                               _lib.ptr(loss.seed) if inside else None, loss.p if inside else 0,
                               _lib.ptr(loss.partials) if inside else None, d_pred.data_ptr() if inside else None,
                               loss.value.data_ptr() if inside else None, None, weights.max_union, _lib.stream_ptr())
        _lib.check(rc, "pit_decoder_bwd")
        d_head = hg.finish(head, scale)
        # weight gradients: the reductions over all rows are postponed and carried by a later launch of the pass (_dw_defer) in the
        # in-place mode, performed now otherwise
        grads, inplace = _mlp_grad_slots(ctx.params, (w1.shape, (d,), w2.shape, (n2,)), ctx.needs_input_grad[9:13], dev)
        d_w = _dw_deliver(_params_job(x, h, d_pred, dz1, grads, (rows, n_head * d, d, n2), 0, 0), inplace, dev)
        dv = dvals if ctx.needs_input_grad[0] else None
        # (forward's inputs: values, head, then plan, n_head, head_is_scale, head_param, weights, params, loss - and w1, b1, w2, b2)
        return (dv, d_head) + (None,) * 7 + d_w


@torch.compiler.disable
def decoder_apply(values: torch.Tensor, lmda: torch.Tensor, plan: MeshPlan, n_head: int, mlp, head_is_scale: bool = False) -> torch.Tensor:
    """pit.decoder (pit.py:124-127) as one launch per direction: de(posatt_cross(mesh_out, mesh_ltt, values)) with
    ``mlp`` = de's (w1, b1, w2, b2).  The caller checked edge_fusion_supported(plan, ..., needs_union=True)."""
    param = lmda if isinstance(lmda, torch.nn.Parameter) else None
    c = host_head_scale(lmda) if (not head_is_scale and get_head_scale_route() == "host") else None
    need_q = torch.is_grad_enabled() and (values.requires_grad or lmda.requires_grad or any(t.requires_grad for t in mlp))
    # the step's weights: formed under the encoder-side launch when pit.encoder requested them for exactly this plan / lmda / route
    weights = getattr(_STEP, "dec_ready", None)
    _STEP.dec_ready = None
    if weights is None or weights.key != _dec_weights_key(plan, lmda, c, n_head, head_is_scale, mlp[0]) or (need_q and weights.qw is None):
        weights = _new_decoder_weights(plan, lmda, c, n_head, head_is_scale, need_q, mlp[0])
        _launch_decoder_weights(weights)
    loss = getattr(_STEP, "loss", None)
    if loss is not None:
        _STEP.loss = None                        # (one decoder per step takes it)
        if not loss.fits(values.shape[0], plan.n_out, mlp[2].shape[0]):
            loss = None
        else:
            _STEP.loss_issued = loss
    return _Decoder.apply(values, lmda.reshape(-1), plan, n_head, head_is_scale, param, weights, tuple(mlp), loss, *mlp)


# ------------------------------------------------------------------------------------------------ folded decoder (round 6)
# pit.decoder = de(up(values)) with de.mlp1 folded into the values (csrc/pit_fold.hip):
#     vw = values @ W'^T  (W' = W1's memory as an (H*hid, hid) matrix: head-interleaved columns)      _Linear, n_in rows
#     z  = sum_h P_h vw_h                                                                              _FoldAtt (batch-free meshes)
#          or posatt_cross on vw for one head (any mesh kind: the candidate-list / union-tile kernels)  _PosAtt
#     y  = gelu(z + b1) @ W2^T + b2                                                                     _ThinTail
# The (batch, n_out, H*hid) tensor of pit.py:125 and the three GEMMs on its rows are gone; nothing of size n_out x hid is saved
# except z itself.  PIT_FOLD_DECODER=0: the round-5 path (attention output materialised, kaiming_mlp kernels).
FOLD_DECODER = os.environ.get("PIT_FOLD_DECODER", "1") != "0"
# d(values) of the fold attention WITHOUT atomics (per-slab tiles + a fixed-order reduction: the same bits on every run): "auto" - when
# the tiles take at most 64 MB (Vorticity b=20: 42 MB, no slower than the atomic adds; Darcy b=256: 126 MB, 1.3 % slower) or under
# torch.use_deterministic_algorithms; "1" always; "0" never (fp32 atomic adds into a zeroed buffer)
FOLD_TILES = os.environ.get("PIT_FOLD_TILES", "auto")
FOLD_TILES_MAX_BYTES = 64 << 20


def _fold_tiles(nbytes: int) -> bool:
    if FOLD_TILES in ("0", False):
        return False
    return FOLD_TILES in ("1", True) or nbytes <= FOLD_TILES_MAX_BYTES or torch.are_deterministic_algorithms_enabled()
# hid 32 / 64 models on batch-free meshes: rows (batch x output points) from which pit.decoder prefers the folded decoder to the
# fused one-launch-per-direction decoder of csrc/pit_edge.hip (which recomputes nothing but pays 16-row slabs: one gather of the
# union's value rows and one pass of atomic adds per 16 rows)
FOLD_EDGE_ROWS = int(os.environ.get("PIT_FOLD_EDGE_ROWS", "300000"))      # Darcy: batch 128 0.974 vs 0.979 ms, batch 256 1.789 vs 1.711
_ZERO_BIAS = {}


def _zero_bias(n: int, device) -> torch.Tensor:
    key = (device.index, n)
    z = _ZERO_BIAS.get(key)
    if z is None:
        z = _ZERO_BIAS[key] = torch.zeros((n,), device=device, dtype=torch.float32)
        _pin(z)
    return z


def _rows2d(t: torch.Tensor) -> torch.Tensor:
    """(b, L, D) tensor whose (b*L) rows are uniformly strided with unit channel stride (copy only if they are not)."""
    t = _row_view(t)
    if t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


class _Linear(torch.autograd.Function):
    """y = x @ W'^T without bias, W' = ``w``'s memory read as a (w.numel() / d, d) row-major matrix (d = x's width): for the fold,
    ``w`` is de.mlp1.weight (hid, H*hid) and W' its (H*hid, hid) view - row n*H + h of W' is W1[n, h*hid:(h+1)*hid]."""

    @staticmethod
    def forward(ctx, x, w, w_param):
        _need_gpu(x, w)
        x = _rows2d(x)
        b, j, d = x.shape
        wc = w.detach()
        if not wc.is_contiguous() or wc.data_ptr() % 16:
            wc = wc.contiguous()
        n_out = wc.numel() // d
        y = torch.empty((b, j, n_out), device=x.device, dtype=torch.float32)
        ctx.math = _math_code()
        rc = _lib.lib().pit_linear_fwd(x.data_ptr(), x.stride(1), b * j, d, n_out, wc.data_ptr(), _zero_bias(n_out, x.device).data_ptr(),
                                       y.data_ptr(), n_out, ctx.math, _lib.stream_ptr())
        _lib.check(rc, "pit_linear_fwd")
        ctx.w_param = w_param
        ctx.save_for_backward(x, wc)
        return y

    @staticmethod
    def backward(ctx, d_y):
        x, wc = ctx.saved_tensors
        b, j, d = x.shape
        n_out = wc.numel() // d
        d_y = d_y.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_x = torch.empty((b, j, d), device=x.device, dtype=torch.float32) if need_x else None
        slot = _grad_slot(ctx.w_param) if (need_w and ctx.w_param is not None and ctx.w_param.data_ptr() == wc.data_ptr()) else None
        d_w = slot if slot is not None else (torch.empty_like(wc) if need_w else None)
        rc = _lib.lib().pit_linear_bwd(x.data_ptr(), x.stride(1), b * j, d, n_out, wc.data_ptr(), d_y.data_ptr(), n_out,
                                       _lib.ptr(d_x), d, _lib.ptr(d_w), 1 if slot is not None else 0, ctx.math, _lib.stream_ptr())
        _lib.check(rc, "pit_linear_bwd")
        return d_x, (None if slot is not None else d_w), None


class FoldWeights:
    """The softmax weights of one step on a fold plan (pit_fold_weights): pw / qw (n_slabs*H, rows, um), the head scales c."""
    __slots__ = ("pw", "qw", "scale", "keep", "pw16", "qw16")


def _new_fold_weights(plan: MeshPlan, head, scale_in, n_head: int, head_is_scale: bool, need_q: bool) -> FoldWeights:
    sp, max_union, _t, max_count = plan.fold_plan()
    um = 32 if max_union <= 32 else (48 if max_union <= 48 else 64)
    dev = plan.mesh_out.device
    w = FoldWeights()
    w.pw = torch.empty((sp.n_slabs * n_head, sp.rows, um), device=dev, dtype=torch.float32)
    w.qw = torch.empty((sp.n_slabs * n_head, sp.rows, um), device=dev, dtype=torch.float32) if need_q else None
    w.scale = torch.empty((n_head,), device=dev, dtype=torch.float32)
    k_head = scale_in if scale_in is not None else head
    w.keep = (k_head, plan, sp)
    # bf16 math mode: the fold launches read the tiles as bf16 (every workgroup of every sample and column chunk used to round the
    # same fp32 tiles on their way into LDS; now half the bytes per pass and nothing to round)
    bf = _math_code() == MATH_MODES["bf16"]
    w.pw16 = torch.empty((sp.n_slabs * n_head, sp.rows, um), device=dev, dtype=torch.bfloat16) if bf else None
    w.qw16 = torch.empty((sp.n_slabs * n_head, sp.rows, um), device=dev, dtype=torch.bfloat16) if (bf and need_q) else None
    rc = _lib.lib().pit_fold_weights(ctypes.byref(sp), k_head.data_ptr(), 1 if (scale_in is not None or head_is_scale) else 0, n_head,
                                     max_union, max_count, w.pw.data_ptr(), _lib.ptr(w.qw), w.scale.data_ptr(), _lib.ptr(w.pw16),
                                     _lib.ptr(w.qw16), _lib.stream_ptr())
    _lib.check(rc, "pit_fold_weights")
    return w


def fold_att_supported(plan: MeshPlan, n_head: int, dim: int, batch: int) -> bool:
    """The fold attention launches cover this layer: a masked cross attention on a batch-free mesh pair with complete candidate
    lists whose unions fit a tile for slabs of at least 64 rows, 1-2 heads, a width that is a multiple of 64."""
    if plan.mesh_batch != 1 or plan.self_attn or not plan.masked or plan.nbr_idx is None or plan.sdim > 3:
        return False
    if torch.are_deterministic_algorithms_enabled() and FOLD_TILES in ("0", False):         # (d(values) as fp32 atomic adds)
        return False
    if not _lib.lib().pit_fold_supported(int(n_head), int(dim), int(batch), int(plan.n_out), int(plan.n_in)):
        return False
    return plan.fold_plan() is not None


class _FoldAtt(torch.autograd.Function):
    """z[b, n, c] = sum_h sum_j P_h[n, j] vw[b, j, c*H + h] on a batch-free mesh pair (pit_fold_att_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, vw, head, plan: MeshPlan, n_head: int, head_is_scale: bool, head_param, scale_in, out_bf16: bool,
                need_q: bool = True):
        _need_gpu(vw, head)
        vw = _rows2d(vw)
        b, j, hd = vw.shape
        d = hd // n_head
        if j != plan.n_in:
            raise RuntimeError(f"inputs have {j} points but mesh_in has {plan.n_in}")
        head = head.detach().reshape(-1).contiguous()
        ctx.math = _math_code()
        out_bf16 = bool(out_bf16 and ctx.math == MATH_MODES["bf16"])
        w = _new_fold_weights(plan, head, scale_in, n_head, head_is_scale, need_q)
        sp, max_union = plan.fold_plan()[0], plan.fold_plan()[1]
        z = torch.empty((b, plan.n_out, d), device=vw.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
        rc = _lib.lib().pit_fold_att_fwd(ctypes.byref(sp), vw.data_ptr(), vw.stride(1), vw.stride(0), b, n_head, d,
                                         (w.pw16 if w.pw16 is not None else w.pw).data_ptr(),
                                         z.data_ptr(), z.stride(1), z.stride(0), max_union,
                                         ctx.math | (IO_OUT_BF16 if out_bf16 else 0), _lib.stream_ptr())
        _lib.check(rc, "pit_fold_att_fwd")
        ctx.plan, ctx.n_head, ctx.head_is_scale, ctx.head_param, ctx.w = plan, n_head, head_is_scale, head_param, w
        ctx.save_for_backward(vw, head)
        return z

    @staticmethod
    def backward(ctx, dz):
        vw, head = ctx.saved_tensors
        plan, n_head, w = ctx.plan, ctx.n_head, ctx.w
        b, j, hd = vw.shape
        d = hd // n_head
        dz = _row_view(dz)
        _need_gpu_bf16_ok(dz)
        io = IO_DOUT_BF16 if dz.dtype == torch.bfloat16 else 0
        if dz.stride(1) % 4 or dz.stride(0) % 4 or dz.data_ptr() % 16:
            dz = dz.contiguous()
        need_v, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_h and w.qw is None:
            raise RuntimeError("fold attention: d(lmda) requested but the forward ran without grad mode")
        # d(values): per-slab sums into tiles + a fixed-order reduction per key (no atomics, nothing to zero: FOLD_TILES), or fp32
        # atomic adds into a zeroed buffer
        fp = plan.fold_plan()
        tiles = rev_ptr = rev_ent = None
        if need_v and _fold_tiles(4 * b * fp[0].n_slabs * SLAB_UNION_MAX * hd):
            tiles = torch.empty((b, fp[0].n_slabs, SLAB_UNION_MAX, hd), device=vw.device, dtype=torch.float32)
            rev_ptr, rev_ent = fp[2][4], fp[2][5]
            d_vw = torch.empty((b, j, hd), device=vw.device, dtype=torch.float32)
        else:
            d_vw = torch.zeros((b, j, hd), device=vw.device, dtype=torch.float32) if need_v else None
        hg = _HeadGrad(ctx.head_param, need_h, n_head, vw.device, ctx.head_is_scale)
        _dw_run_pending(vw.device)                   # (a postponed weight-gradient job: nothing here carries it)
        sp, max_union = plan.fold_plan()[0], plan.fold_plan()[1]
        pw = w.pw16 if w.pw16 is not None else w.pw    # (bf16 math mode: the bf16 tiles)
        qw = (w.qw16 if w.qw16 is not None else pw) if w.pw16 is not None else (w.qw if w.qw is not None else w.pw)      # (read only for d(scale))
        rc = _lib.lib().pit_fold_att_bwd(ctypes.byref(sp), vw.data_ptr(), vw.stride(1), vw.stride(0), b, n_head, d, pw.data_ptr(),
                                         qw.data_ptr(), dz.data_ptr(), dz.stride(1), dz.stride(0),
                                         _lib.ptr(d_vw), hd, j * hd, _lib.ptr(hg.work), _lib.ptr(tiles), _lib.ptr(rev_ptr),
                                         _lib.ptr(rev_ent), max_union, ctx.math | io, _lib.stream_ptr())
        _lib.check(rc, "pit_fold_att_bwd")
        # (forward's inputs: vw, head, then plan, n_head, head_is_scale, head_param, scale_in, out_bf16, need_q)
        return (d_vw, hg.finish(head, w.scale)) + (None,) * 7


_TAIL_WS = {}       # (device index, stream) -> the thin tail's slotted partial sums (self-cleaning)


def _tail_scratch(device) -> torch.Tensor:
    key = _ws_key(device)
    ws = _TAIL_WS.get(key)
    if ws is None:
        ws = _TAIL_WS[key] = torch.zeros((_lib.lib().pit_thin_tail_scratch_floats(),), device=device, dtype=torch.float32)
        _pin(ws)
    return ws


class _ThinTail(torch.autograd.Function):
    """y = gelu(z + b1) @ W2^T + b2 for out_dim <= 4 (pit_thin_tail_fwd / _bwd): z fp32 or bf16, nothing but z is saved."""

    @staticmethod
    def forward(ctx, z, b1, w2, b2, params):
        _need_gpu_bf16_ok(z)
        _need_gpu(b1, w2, b2)
        z = _row_view(z)
        if z.stride(0) != z.shape[1] * z.stride(1) or z.stride(1) % 4 or z.data_ptr() % 16:
            z = z.contiguous()
        b, n, d = z.shape
        n2 = w2.shape[0]
        b1c, w2c, b2c = (t.detach().contiguous() for t in (b1, w2, b2))
        y = torch.empty((b, n, n2), device=z.device, dtype=torch.float32)
        ctx.math = _math_code() | (IO_X_BF16 if z.dtype == torch.bfloat16 else 0)
        rc = _lib.lib().pit_thin_tail_fwd(z.data_ptr(), z.stride(1), b * n, d, n2, b1c.data_ptr(), w2c.data_ptr(), b2c.data_ptr(),
                                          y.data_ptr(), n2, ctx.math, _lib.stream_ptr())
        _lib.check(rc, "pit_thin_tail_fwd")
        ctx.params = params
        ctx.save_for_backward(z, b1c, w2c)
        return y

    @staticmethod
    def backward(ctx, d_y):
        z, b1c, w2c = ctx.saved_tensors
        b, n, d = z.shape
        n2 = w2c.shape[0]
        d_y = d_y.reshape(b * n, n2)
        if d_y.stride(1) != 1 or d_y.stride(0) < n2:
            d_y = d_y.contiguous()
        dz = torch.empty((b, n, d), device=z.device, dtype=z.dtype)
        slots = [_grad_slot(q) if isinstance(q, torch.nn.Parameter) else None for q in ctx.params]
        inplace = all(t is not None for t in slots) and all(ctx.needs_input_grad[1:4])
        if inplace:
            d_b1, d_w2, d_b2 = slots
        else:
            d_b1, d_w2, d_b2 = (torch.zeros_like(t) for t in (b1c, w2c, b1c[:n2]))
        rc = _lib.lib().pit_thin_tail_bwd(z.data_ptr(), z.stride(1), b * n, d, n2, b1c.data_ptr(), w2c.data_ptr(), d_y.data_ptr(),
                                          d_y.stride(0), dz.data_ptr(), d, d_b1.data_ptr(), d_w2.data_ptr(), d_b2.data_ptr(),
                                          _tail_scratch(z.device).data_ptr(), ctx.math, _lib.stream_ptr())
        _lib.check(rc, "pit_thin_tail_bwd")
        if inplace:
            return dz, None, None, None, None
        return dz, d_b1, d_w2, d_b2, None


@torch.compiler.disable
def fold_decoder_apply(values: torch.Tensor, lmda: torch.Tensor, plan: MeshPlan, n_head: int, mlp, use_fold_att: bool) -> torch.Tensor:
    """pit.decoder (pit.py:124-127) with de.mlp1 folded into the values (see the section comment); ``mlp`` = de's
    (w1, b1, w2, b2).  ``use_fold_att``: the fold attention launches (batch-free meshes, fold_att_supported) - else one head on
    the candidate-list / union-tile kernels of posatt_apply."""
    w1, b1, w2, b2 = mlp
    vw = _Linear.apply(values, w1, w1 if isinstance(w1, torch.nn.Parameter) else None)
    bf16 = get_math_mode() == "bf16" and BF16_STORAGE
    if use_fold_att:
        param = lmda if isinstance(lmda, torch.nn.Parameter) else None
        c = host_head_scale(lmda) if get_head_scale_route() == "host" else None
        need_q = torch.is_grad_enabled() and lmda.requires_grad        # (Q = P (m - mbar): read by d(scale) only)
        z = _FoldAtt.apply(vw, lmda.reshape(-1), plan, n_head, False, param, c, bf16, need_q)
    else:
        z = posatt_apply(vw, lmda, plan, n_head, concat=False, out_bf16=bf16)
    return _ThinTail.apply(z, b1, w2, b2, (b1, w2, b2))


class _Encoder(torch.autograd.Function):
    """pit.encoder (pit.py:108-112): posatt_cross_* (mesh_in -> mesh_ltt) + kaiming_mlp `en_layer` + gelu."""

    @staticmethod
    def forward(ctx, values, head, plan: MeshPlan, n_head: int, head_is_scale: bool, head_param, scale_in, params, coord_dims: int,
                concat_heads: int, wjob, clear, w1, b1, w2, b2, djob=None, need=True):
        _need_gpu(values, head, w1, b1, w2, b2)
        values = _row_view(values)
        b, j, dv = values.shape
        d = w1.shape[0]
        kd = int(coord_dims)
        k0 = n_head * (kd + dv)
        dev = values.device
        sp = plan.slab_plan()[0]
        head = head.detach().reshape(-1).contiguous()
        k_head, k_is_scale = (scale_in, True) if scale_in is not None else (head, head_is_scale)
        w1c, b1c, w2c, b2c = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        rows = b * plan.n_out
        buf = None
        if concat_heads > 0:
            buf = torch.empty((rows, (1 + concat_heads) * d), device=dev, dtype=torch.float32)
            y = buf[:, :d]
        else:
            y = torch.empty((rows, d), device=dev, dtype=torch.float32)
        x = z1 = h = z2 = rowstat = scale = None
        if need:
            x = torch.empty((rows, k0), device=dev, dtype=torch.float32)
            z1 = torch.empty((rows, d), device=dev, dtype=torch.float32)
            h = torch.empty((rows, d), device=dev, dtype=torch.float32)
            z2 = torch.empty((rows, d), device=dev, dtype=torch.float32)
            rowstat = torch.empty((n_head, plan.n_out, 4), device=dev, dtype=torch.float32)
            scale = torch.empty((n_head,), device=dev, dtype=torch.float32)
        rc = _lib.lib().pit_encoder_fwd(ctypes.byref(sp), plan.mesh_in.data_ptr(), plan.sdim, kd, values.data_ptr(), values.stride(1),
                                        values.stride(0), dv, b, n_head, d, k_head.data_ptr(), 1 if k_is_scale else 0,
                                        w1c.data_ptr(), b1c.data_ptr(), w2c.data_ptr(), b2c.data_ptr(), _lib.ptr(x), _lib.ptr(z1),
                                        _lib.ptr(h), _lib.ptr(z2), y.data_ptr(), y.stride(0), _lib.ptr(rowstat), _lib.ptr(scale),
                                        _lib.ptr(clear), clear.numel() if clear is not None else 0,
                                        ctypes.cast(ctypes.pointer(wjob.job), ctypes.c_void_p) if wjob is not None else None,
                                        ctypes.cast(ctypes.pointer(djob.job), ctypes.c_void_p) if djob is not None else None,
                                        _lib.stream_ptr())
        _lib.check(rc, "pit_encoder_fwd")
        ctx.plan, ctx.n_head, ctx.head_is_scale, ctx.head_param, ctx.params, ctx.kd = plan, n_head, head_is_scale, head_param, params, kd
        ctx.keep = (values, head, w1c, w2c, x, z1, h, z2, rowstat, scale)
        out = y.reshape(b, plan.n_out, d)
        if buf is None:
            return out
        buf = buf.reshape(b, plan.n_out, (1 + concat_heads) * d)
        ctx.mark_non_differentiable(buf)
        ctx.set_materialize_grads(False)
        return out, buf

    @staticmethod
    def backward(ctx, d_y, _d_buf=None):
        values, head, w1, w2, x, z1, h, z2, rowstat, scale = ctx.keep
        plan, n_head, kd = ctx.plan, ctx.n_head, ctx.kd
        b, j, dv = values.shape
        d, rows = w1.shape[0], b * plan.n_out
        dev = values.device
        sp = plan.slab_plan()[0]
        if d_y is None:
            d_y = torch.zeros((rows, d), device=dev, dtype=torch.float32)
        d_y2 = d_y.reshape(rows, d)
        if d_y2.stride(1) != 1 or d_y2.stride(0) < d:
            d_y2 = d_y2.contiguous()
        scratch = torch.empty((rows * 2 * d,), device=dev, dtype=torch.float32)
        # (the launch always reduces d(scale): accumulators of its own when lmda needs no gradient)
        hg = _HeadGrad(ctx.head_param, ctx.needs_input_grad[1], n_head, dev, ctx.head_is_scale, always_accumulators=True)
        rc = _lib.lib().pit_encoder_bwd(ctypes.byref(sp), plan.mesh_in.data_ptr(), plan.sdim, kd, values.data_ptr(), values.stride(1),
                                        values.stride(0), dv, b, n_head, d, scale.data_ptr(), rowstat.data_ptr(), w1.data_ptr(),
                                        w2.data_ptr(), z1.data_ptr(), z2.data_ptr(), d_y2.data_ptr(), d_y2.stride(0),
                                        scratch.data_ptr(), _lib.ptr(hg.work), _lib.stream_ptr())
        _lib.check(rc, "pit_encoder_bwd")
        d_head = hg.finish(head, scale)
        grads, inplace = _mlp_grad_slots(ctx.params, (w1.shape, (d,), w2.shape, (d,)), ctx.needs_input_grad[12:16], dev)
        d_w = _dw_deliver(_params_job(x, h, d_y2, scratch, grads, (rows, n_head * (kd + dv), d, d), 1, 0), inplace, dev)
        # (forward's inputs: values, head, then plan, n_head, head_is_scale, head_param, scale_in, params, coord_dims, concat_heads,
        # wjob, clear - then w1, b1, w2, b2 - then djob, need)
        return (None, d_head) + (None,) * 10 + d_w + (None, None)


@torch.compiler.disable
def encoder_apply(values: torch.Tensor, lmda: torch.Tensor, plan: MeshPlan, n_head: int, mlp, concat_heads: int = 0,
                  head_is_scale: bool = False, early=None) -> torch.Tensor:
    """pit.encoder (pit.py:108-112) as one launch per direction: gelu(en_layer(posatt_cross(mesh_ltt, mesh_in, values))); ``values``
    may be tagged by tag_coords (the coordinate channels then come from the mesh).  ``early``: early_block_weights(...) whose job
    this launch carries.  The inputs get no gradient (the caller checked that they need none)."""
    param = lmda if isinstance(lmda, torch.nn.Parameter) else None
    c = host_head_scale(lmda) if (not head_is_scale and get_head_scale_route() == "host") else None
    coords = getattr(values, "_pit_coords", None)
    kd = plan.sdim if coords is not None else 0
    wjob = None
    if early is not None and getattr(_STEP, "fwd_job", None) is early:
        _STEP.fwd_job = None
        wjob = early
    clear = getattr(_STEP, "clear", None)
    if clear is not None:
        _STEP.clear = None                       # (zeroed by this launch: the step's loss launch need not)
    djob = getattr(_STEP, "dec_job", None)       # the decoder's weights of this forward ride in this launch (early_decoder_weights)
    _STEP.dec_job = None
    res = _Encoder.apply(values.detach(), lmda.reshape(-1), plan, n_head, head_is_scale, param, c, tuple(mlp), kd, int(concat_heads),
                         wjob, clear, *mlp, djob,
                         torch.is_grad_enabled() and (lmda.requires_grad or any(t.requires_grad for t in mlp)))
    _STEP.dec_ready = djob
    if concat_heads <= 0:
        return res
    y, buf = res
    y._pit_concat = buf
    return y


class _RelLpLoss(torch.autograd.Function):
    """RelLpNorm (utils.py:80-98), optionally fused with the per-pixel affine
    de-normalisation of the prediction (utils.py:25-34).

    With ``unit_seed`` (the tensor of ones a training step seeds its backward pass with) the forward
    launch also writes the gradients for d loss = 1; backward returns them without a launch when
    it is indeed handed that seed, and falls back to the general backward kernel otherwise.
    ``clear`` is a tensor the same launch zeroes (the step's flat gradient accumulators)."""

    @staticmethod
    def forward(ctx, pred, true, out_dim: int, p: int, scale, shift, unit_seed=None, clear=None):
        _need_gpu(pred, true, scale, shift)
        b = true.size(0)
        t = true.reshape(b, -1, out_dim).contiguous()
        q = pred.reshape(b, -1, out_dim).contiguous()
        if t.shape != q.shape:
            raise RuntimeError(f"true {tuple(true.shape)} and pred {tuple(pred.shape)} do not match")
        npts = t.shape[1]
        sc = scale.reshape(npts, out_dim).contiguous() if scale is not None else None
        sh = shift.reshape(npts, out_dim).contiguous() if shift is not None else None
        norms = torch.empty((b, out_dim, 2), device=t.device, dtype=torch.float32)
        loss = torch.empty((), device=t.device, dtype=torch.float32)
        wkey = _ws_key(t.device) + (b * out_dim,)             # PIT_REL_LP_WS_FLOATS(batch, nch)
        ws = _LOSS_WS.get(wkey)
        if ws is None:
            ws = _LOSS_WS[wkey] = torch.zeros(4 + 5 * b * out_dim, device=t.device, dtype=torch.float32)
        if _capturing():
            _pin(ws)
        unit_p = unit_t = None
        # reproducible mode: the entry whose sums all run in a fixed order (a series is never split, the pairs in index order)
        fwd_grad = "pit_rel_lp_loss_fwd_grad_ordered" if reproducible_wanted() else "pit_rel_lp_loss_fwd_grad"
        if unit_seed is not None or clear is not None or fwd_grad.endswith("_ordered"):
            if unit_seed is not None:
                unit_p = torch.empty_like(q) if pred.requires_grad else None
                unit_t = torch.empty_like(t) if true.requires_grad else None
            if clear is not None and (not clear.is_contiguous() or clear.dtype != torch.float32):
                raise RuntimeError("clear must be a contiguous fp32 tensor")
            rc = getattr(_lib.lib(), fwd_grad)(t.data_ptr(), q.data_ptr(), _lib.ptr(sc), _lib.ptr(sh), b, npts,
                                               out_dim, int(p), norms.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                               _lib.ptr(unit_p), _lib.ptr(unit_t), _lib.ptr(clear),
                                               clear.numel() if clear is not None else 0, _lib.stream_ptr())
            _lib.check(rc, fwd_grad)
        else:
            rc = _lib.lib().pit_rel_lp_loss_fwd(t.data_ptr(), q.data_ptr(), _lib.ptr(sc), _lib.ptr(sh), b, npts,
                                                out_dim, int(p), norms.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                                _lib.stream_ptr())
            _lib.check(rc, "pit_rel_lp_loss_fwd")
        ctx.meta = (b, npts, out_dim, int(p), pred.shape, true.shape)
        ctx.save_for_backward(t, q, norms, sc if sc is not None else norms, sh if sh is not None else norms)
        ctx.affine = sc is not None
        ctx.unit = (unit_seed.data_ptr() if unit_seed is not None else 0, unit_p, unit_t)
        return loss

    @staticmethod
    def backward(ctx, g):
        t, q, norms, sc, sh = ctx.saved_tensors
        b, npts, out_dim, p, shape, tshape = ctx.meta
        need_p, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_p or need_t):
            return None, None, None, None, None, None, None, None
        seed_ptr, unit_p, unit_t = ctx.unit
        if seed_ptr and g.data_ptr() == seed_ptr and (unit_p is not None or not need_p) and \
                (unit_t is not None or not need_t):
            # d loss is the step's tensor of ones: the forward launch already wrote these gradients
            return (unit_p.reshape(shape) if need_p else None), (unit_t.reshape(tshape) if need_t else None), \
                None, None, None, None, None, None
        g = g.contiguous()
        d_pred = torch.empty_like(q) if need_p else None
        d_true = torch.empty_like(t) if need_t else None
        rc = _lib.lib().pit_rel_lp_loss_bwd(t.data_ptr(), q.data_ptr(), sc.data_ptr() if ctx.affine else 0,
                                            sh.data_ptr() if ctx.affine else 0, b, npts, out_dim, p,
                                            norms.data_ptr(), g.data_ptr(), _lib.ptr(d_pred), _lib.ptr(d_true),
                                            _lib.stream_ptr())
        _lib.check(rc, "pit_rel_lp_loss_bwd")
        return (d_pred.reshape(shape) if need_p else None), (d_true.reshape(tshape) if need_t else None), \
            None, None, None, None, None, None


class _FusedLoss(torch.autograd.Function):
    """The loss node of a step whose decoder launches carry the loss (LossSpec): no launch in either direction.  The forward
    returns the scalar the decoder BACKWARD launch will write (a training step reads its loss after the pass); the backward hands
    a token tensor down the graph that pit.decoder's backward recognises by its address - it reaches it through views only.
    THE RETURNED TENSOR IS VALID ONLY AFTER backward() HAS RUN: until then it is uninitialised memory (initialising it would be a
    launch - the step has fourteen), so nothing may be derived from it in the forward (scaling, logging, a finite check).  Only
    engine.TrainStep / ops.step_state(loss=...) open this path, and they read the loss after the pass; every other caller of
    rel_lp_loss gets _RelLpLoss, whose value is computed in the forward."""

    @staticmethod
    def forward(ctx, pred, spec: LossSpec):
        ctx.spec, ctx.pred_shape = spec, pred.shape
        return spec.value

    @staticmethod
    def backward(ctx, g):
        spec = ctx.spec
        spec.seed = g.contiguous()
        spec.token = torch.empty_like(spec.pred)           # never written, never read: its address is the message
        return spec.token.view(ctx.pred_shape), None


def _take_fused_loss(true, pred, out_dim: int, p: int, scale, shift):
    """The LossSpec the running step's decoder accumulated for exactly this loss call, or None."""
    spec = getattr(_STEP, "loss_issued", None)
    if spec is None or spec.pred is None:
        return None
    _STEP.loss_issued = None
    same = lambda a, b_: (a is None and b_ is None) or (a is not None and b_ is not None and a.data_ptr() == b_.data_ptr())
    npts = spec.true.shape[1]
    sc = scale.reshape(npts, out_dim) if scale is not None and scale.numel() == npts * out_dim else scale
    sh = shift.reshape(npts, out_dim) if shift is not None and shift.numel() == npts * out_dim else shift
    ok = (int(p) == spec.p and int(out_dim) == spec.out_dim and pred.requires_grad and pred.is_contiguous()
          and pred.data_ptr() == spec.pred.data_ptr() and pred.numel() == spec.pred.numel()
          and true.numel() == spec.true.numel() and true.is_contiguous() and true.data_ptr() == spec.true.data_ptr()
          and (sc is None or sc.is_contiguous()) and (sh is None or sh.is_contiguous())
          and same(sc, spec.scale) and same(sh, spec.shift))
    return spec if ok else None


@torch.compiler.disable
def rel_lp_loss(true, pred, out_dim: int, p: int, pred_scale=None, pred_shift=None, unit_seed=None,
                clear=None) -> torch.Tensor:
    """sum_b mean_c ||true - pred'||_p / ||true||_p with pred' = pred*pred_scale + pred_shift.
    ``unit_seed`` / ``clear``: see _RelLpLoss (used by engine.TrainStep to save two launches).  Inside a step whose fused decoder
    already accumulated this very loss (step_state(loss=...)), no launch at all: see _FusedLoss."""
    spec = _take_fused_loss(true, pred, out_dim, p, pred_scale, pred_shift)
    if spec is not None:
        if clear is not None:
            clear.zero_()
        return _FusedLoss.apply(pred, spec)
    return _RelLpLoss.apply(pred, true, out_dim, p, pred_scale, pred_shift, unit_seed, clear)


_RAGGED_LOSS_WS = {}       # (device index, stream) -> the arrival ticket of pit_rel_lp_loss_ragged_fwd_grad (zero between calls)


class _RelLpLossRagged(torch.autograd.Function):
    """RelLpNorm of every sample truncated to its first lengths[s] points (pit_rel_lp_loss_ragged_*): padded points are
    skipped and get a zero gradient; ``true`` gets none (data).

    With ``unit_seed`` / ``clear`` (see _RelLpLoss: the seed of ones of a training step, its flat gradient accumulators) ONE
    launch - pit_rel_lp_loss_ragged_fwd_grad - writes the norms, the loss, the gradient for d loss = 1 and the zeros; backward
    returns that gradient without a launch when it is handed the seed itself and runs pit_rel_lp_loss_ragged_bwd on the saved
    norms otherwise.  The values are the same bits either way."""

    @staticmethod
    def forward(ctx, pred, true, lengths, out_dim: int, p: int, unit_seed=None, clear=None):
        _need_gpu(pred, true)
        b = true.size(0)
        t = true.detach().reshape(b, -1, out_dim).contiguous()
        q = pred.detach().reshape(b, -1, out_dim).contiguous()
        if t.shape != q.shape:
            raise RuntimeError(f"true {tuple(true.shape)} and pred {tuple(pred.shape)} do not match")
        npts = t.shape[1]
        norms = torch.empty((b, out_dim, 2), device=t.device, dtype=torch.float32)
        loss = torch.empty((), device=t.device, dtype=torch.float32)
        unit_p = None
        if unit_seed is None and clear is None:
            rc = _lib.lib().pit_rel_lp_loss_ragged_fwd(t.data_ptr(), q.data_ptr(), lengths.data_ptr(), b, npts, out_dim, int(p),
                                                       norms.data_ptr(), loss.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "pit_rel_lp_loss_ragged_fwd")
        else:
            if clear is not None and (not clear.is_contiguous() or clear.dtype != torch.float32):
                raise RuntimeError("clear must be a contiguous fp32 tensor")
            wkey = _ws_key(t.device)
            ws = _RAGGED_LOSS_WS.get(wkey)
            if ws is None:
                ws = _RAGGED_LOSS_WS[wkey] = torch.zeros(4, device=t.device, dtype=torch.int32)
            if _capturing():
                _pin(ws)
            if unit_seed is not None and pred.requires_grad:
                unit_p = torch.empty_like(q)
            rc = _lib.lib().pit_rel_lp_loss_ragged_fwd_grad(t.data_ptr(), q.data_ptr(), lengths.data_ptr(), b, npts, out_dim, int(p),
                                                            norms.data_ptr(), loss.data_ptr(), ws.data_ptr(), _lib.ptr(unit_p),
                                                            _lib.ptr(clear), clear.numel() if clear is not None else 0,
                                                            _lib.stream_ptr())
            _lib.check(rc, "pit_rel_lp_loss_ragged_fwd_grad")
        ctx.meta = (b, npts, out_dim, int(p), pred.shape)
        ctx.save_for_backward(t, q, norms, lengths)
        ctx.unit = (unit_seed.data_ptr() if unit_seed is not None else 0, unit_p)
        return loss

    @staticmethod
    def backward(ctx, g):
        t, q, norms, lengths = ctx.saved_tensors
        b, npts, out_dim, p, shape = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None, None
        seed_ptr, unit_p = ctx.unit
        if seed_ptr and g.data_ptr() == seed_ptr and unit_p is not None:
            # d loss is the step's tensor of ones: the forward launch already wrote this gradient
            return unit_p.reshape(shape), None, None, None, None, None, None
        g = g.contiguous()
        d_pred = torch.empty_like(q)
        rc = _lib.lib().pit_rel_lp_loss_ragged_bwd(t.data_ptr(), q.data_ptr(), lengths.data_ptr(), b, npts, out_dim, p,
                                                   norms.data_ptr(), g.data_ptr(), d_pred.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_rel_lp_loss_ragged_bwd")
        return d_pred.reshape(shape), None, None, None, None, None, None


@torch.compiler.disable
def rel_lp_loss_ragged(true, pred, lengths, out_dim: int, p: int, unit_seed=None, clear=None) -> torch.Tensor:
    """sum_s mean_c ||true_s - pred_s||_p / ||true_s||_p over the first lengths[s] points of every sample.
    ``unit_seed`` / ``clear``: see _RelLpLossRagged (used by engine.TrainStep: no loss-backward launch, no memset)."""
    if torch.is_grad_enabled() and true.requires_grad:
        raise NotImplementedError("RelLpNorm with lengths gives `true` no gradient (it is data)")
    _need_gpu(pred, true)
    lengths = as_lengths(lengths, pred.device, true.size(0))
    if _capturing():
        _pin(lengths)
    return _RelLpLossRagged.apply(pred, true, lengths, out_dim, p, unit_seed, clear)


_RELMAX_WS = {}


@torch.compiler.disable
def rel_max_norm(true: torch.Tensor, pred: torch.Tensor, out_dim: int) -> torch.Tensor:
    """RelMaxNorm (utils.py:59-77) on device: sum_b mean_c max|true-pred| / max|true|.  Forward only -
    the scripts use it as an evaluation metric under no_grad (train_burgers.py:80, train_naca.py:132)."""
    _need_gpu(true, pred)
    if torch.is_grad_enabled() and (true.requires_grad or pred.requires_grad):
        raise NotImplementedError("RelMaxNorm on device tensors is forward-only (an evaluation metric in the reference "
                                  "scripts): call it under torch.no_grad() or on detached tensors")
    b = true.size(0)
    t = true.detach().reshape(b, -1, out_dim).contiguous()
    q = pred.detach().reshape(b, -1, out_dim).contiguous()
    if t.shape != q.shape:
        raise RuntimeError(f"true {tuple(true.shape)} and pred {tuple(pred.shape)} do not match")
    wkey = _ws_key(t.device)
    ws = _RELMAX_WS.get(wkey)
    if ws is None:
        ws = _RELMAX_WS[wkey] = torch.zeros(2, device=t.device, dtype=torch.float64)
    if _capturing():
        _pin(ws)
    out = torch.empty((), device=t.device, dtype=torch.float32)
    _lib.check(_lib.lib().pit_rel_max_norm(t.data_ptr(), q.data_ptr(), b, t.shape[1], out_dim, out.data_ptr(),
                                           ws.data_ptr(), _lib.stream_ptr()), "pit_rel_max_norm")
    return out


@torch.compiler.disable
def rel_max_norm_ragged(true: torch.Tensor, pred: torch.Tensor, lengths, out_dim: int) -> torch.Tensor:
    """RelMaxNorm (utils.py:59-77) of every sample truncated to its first lengths[s] points: sum_s mean_c max|true-pred| / max|true|
    over the real points; padded points are never read.  Forward only, device tensors only."""
    _need_gpu(true, pred)
    if torch.is_grad_enabled() and (true.requires_grad or pred.requires_grad):
        raise NotImplementedError("RelMaxNorm on device tensors is forward-only (an evaluation metric in the reference "
                                  "scripts): call it under torch.no_grad() or on detached tensors")
    b = true.size(0)
    t = true.detach().reshape(b, -1, out_dim).contiguous()
    q = pred.detach().reshape(b, -1, out_dim).contiguous()
    if t.shape != q.shape:
        raise RuntimeError(f"true {tuple(true.shape)} and pred {tuple(pred.shape)} do not match")
    lengths = as_lengths(lengths, t.device, b)
    if _capturing():
        _pin(lengths)
    out = torch.empty((), device=t.device, dtype=torch.float32)
    _lib.check(_lib.lib().pit_rel_max_norm_ragged(t.data_ptr(), q.data_ptr(), lengths.data_ptr(), b, t.shape[1], out_dim,
                                                  out.data_ptr(), _lib.stream_ptr()), "pit_rel_max_norm_ragged")
    return out


_EVAL_WS = {}              # (device index, stream) -> pit_eval_metrics' workspace (ticket word + slots; the ticket is zero between calls)
EVAL_PARTS = (1, 2, 4, 8, 16, 32, 64)        # the dispatch instances of pit_eval_metrics: workgroups per (sample, channel) series


def eval_parts(batch: int, npts: int, nch: int) -> int:
    """The instance (one of EVAL_PARTS) pit_eval_metrics takes at this shape, read back from the library's workspace size."""
    nbytes = _lib.lib().pit_eval_metrics_workspace(int(batch), int(npts), int(nch))
    if nbytes < 0:
        _lib.check(int(nbytes), "pit_eval_metrics_workspace")
    return (nbytes - 16) // (32 * int(batch) * int(nch))


def new_eval_state(device) -> torch.Tensor:
    """The zeroed state of an evaluation pass (PIT_EVAL_STATE_DOUBLES doubles; see ``eval_metrics``)."""
    return torch.zeros(_lib.EVAL_STATE_DOUBLES, device=device, dtype=torch.float64)


@torch.compiler.disable
def eval_metrics(true: torch.Tensor, pred: torch.Tensor, out_dim: int, p: int, state: torch.Tensor, pred_scale=None,
                 pred_shift=None, lengths=None, n_valid=None, per_sample=None, pred_store=None, advance: bool = True,
                 store_true: bool = False) -> None:
    """One launch of pit_eval_metrics (include/pit_hip.h): RelLpNorm and RelMaxNorm (utils.py:59-98) of every valid sample over
    its real points, added into ``state`` - 8 doubles on the device: [0] sum of RelLp, [1] sum of RelMax, [2] / [3] the worst of
    each, [4] the cursor (samples consumed so far), [5] launches - with no host synchronisation.
      lengths     per-sample point counts (``as_lengths``); padded points are never read
      n_valid     an int32 device scalar: samples from there on are skipped (a partly filled last batch)
      per_sample  (capacity, 2) fp32, last stride 1: row cursor + s receives {RelLp_s, RelMax_s}
      pred_store  (capacity, npts, out_dim) fp32 with contiguous rows: row cursor + s receives pred' (zeros in padded points)
      advance     this launch moves the cursor on by n_valid
      store_true  ``pred_store`` receives ``true`` instead of pred' (callers that put the model output in the ``true`` slot)
    Rows beyond the capacity are not written.  Forward only."""
    _need_gpu(true, pred, pred_scale, pred_shift, per_sample, pred_store)
    if torch.is_grad_enabled() and (true.requires_grad or pred.requires_grad):
        raise NotImplementedError("eval_metrics is forward-only (the evaluation loops of the reference scripts run under "
                                  "no_grad): call it under torch.no_grad() or on detached tensors")
    if not state.is_cuda or state.dtype != torch.float64 or state.numel() != _lib.EVAL_STATE_DOUBLES or not state.is_contiguous():
        raise RuntimeError(f"state must be {_lib.EVAL_STATE_DOUBLES} contiguous float64 values on the HIP device")
    if (pred_scale is None) != (pred_shift is None):
        raise ValueError("pred_scale and pred_shift go together")
    b = true.size(0)
    t = true.detach().reshape(b, -1, out_dim).contiguous()
    q = pred.detach().reshape(b, -1, out_dim).contiguous()
    if t.shape != q.shape:
        raise RuntimeError(f"true {tuple(true.shape)} and pred {tuple(pred.shape)} do not match")
    npts = t.shape[1]
    sc = sh = None
    if pred_scale is not None:
        sc, sh = pred_scale.detach().contiguous(), pred_shift.detach().contiguous()
        if sc.numel() != npts * out_dim or sh.numel() != npts * out_dim:
            raise RuntimeError(f"pred_scale / pred_shift must hold (npts, out_dim) = ({npts}, {out_dim}) values")
    if lengths is not None:
        lengths = as_lengths(lengths, t.device, b)
    if n_valid is not None and (not torch.is_tensor(n_valid) or not n_valid.is_cuda or n_valid.dtype != torch.int32
                                or n_valid.numel() != 1):
        raise RuntimeError("n_valid must be one int32 value on the HIP device")
    capacity = 0
    ps_stride = store_stride = 0
    if per_sample is not None:
        if per_sample.dim() != 2 or per_sample.shape[1] != 2 or per_sample.stride(1) != 1 or per_sample.shape[0] < 1:
            raise RuntimeError("per_sample must be a (capacity, 2) tensor whose rows are contiguous")
        capacity, ps_stride = per_sample.shape[0], per_sample.stride(0)
    if pred_store is not None:
        row = pred_store[0] if pred_store.dim() == 3 and pred_store.shape[0] > 0 else None
        if row is None or tuple(row.shape) != (npts, out_dim) or not row.is_contiguous():
            raise RuntimeError(f"pred_store must be a (capacity, {npts}, {out_dim}) tensor whose rows are contiguous")
        if per_sample is not None and pred_store.shape[0] != capacity:
            raise RuntimeError("per_sample and pred_store must have the same number of rows")
        capacity, store_stride = pred_store.shape[0], pred_store.stride(0)
    nbytes = _lib.lib().pit_eval_metrics_workspace(b, npts, out_dim)
    if nbytes < 0:
        _lib.check(int(nbytes), "pit_eval_metrics_workspace")
    wkey = _ws_key(t.device)
    ws = _EVAL_WS.get(wkey)
    if ws is None or ws.numel() * 8 < nbytes:
        # (a larger shape on this stream: a new zeroed buffer; the old one stays with whatever graph pinned it)
        ws = _EVAL_WS[wkey] = torch.zeros((nbytes + 7) // 8, device=t.device, dtype=torch.float64)
    if _capturing():
        _pin(*[o for o in (ws, lengths, n_valid, sc, sh) if o is not None])
    rc = _lib.lib().pit_eval_metrics(t.data_ptr(), q.data_ptr(), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(lengths), _lib.ptr(n_valid),
                                     b, npts, out_dim, int(p), state.data_ptr(), _lib.ptr(per_sample), ps_stride,
                                     _lib.ptr(pred_store), store_stride, capacity,
                                     (_EVAL_ADVANCE if advance else 0) | (_EVAL_STORE_TRUE if store_true else 0), ws.data_ptr(),
                                     _lib.stream_ptr())
    _lib.check(rc, "pit_eval_metrics")


def new_feed_state(device) -> torch.Tensor:
    """The state of a data feed (``batch_feed``): two int64 on the device, [0] the cursor, [1] the arrival ticket (stays zero)."""
    return torch.zeros(2, device=device, dtype=torch.int64)


@torch.compiler.disable
def batch_feed(src, dst, state: torch.Tensor, rank: int = 0, world: int = 1, drop_last: bool = True, shuffle: bool = True,
               order=None, seed: int = 0, indices=None, n_valid=None) -> None:
    """One launch of pit_batch_feed (include/pit_hip.h): gather this step's samples from the dataset on the device into the
    step's static buffers and move the cursor on, with no host synchronisation.
      src, dst    sequences of 1..8 contiguous device tensors: ``src[f]`` (n_samples, ...) the dataset's field f, ``dst[f]``
                  (batch, ...) its static buffer - the same dtype and the same row; any dtype whose rows are whole 4-byte words
      state       ``new_feed_state``: [0] is the cursor (the number of feeds so far)
      rank, world this rank's shard of the global batch of ``batch * world`` positions
      order       n_samples int32 on the device: the caller's sampler (entries are clamped into range where they are read)
      indices     (batch) int32 on the device: receives the sample index behind every slot
      n_valid     one int32 on the device: receives how many of the slots lie before the end of the epoch
    The sample of a slot: see the header; ``engine.feed_order`` restates the keyed permutation on the host."""
    src, dst = list(src), list(dst)
    if len(src) != len(dst) or not 1 <= len(src) <= _lib.FEED_MAX_FIELDS:
        raise ValueError(f"batch_feed takes 1..{_lib.FEED_MAX_FIELDS} fields, each with a source and a destination")
    for t in src + dst + [state, order, indices, n_valid]:
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise RuntimeError("position_induced_transformer_amd: the data feed runs on the HIP device only; "
                               "got a CPU tensor (move the dataset and the step's buffers to 'cuda')")
    n, batch = src[0].shape[0], dst[0].shape[0]
    rows = []
    for a, b in zip(src, dst):
        if not a.is_contiguous() or not b.is_contiguous():
            raise RuntimeError("batch_feed: every field and every static buffer must be contiguous")
        if a.dtype != b.dtype or a.shape[1:] != b.shape[1:] or a.shape[0] != n or b.shape[0] != batch or a.dim() < 1:
            raise RuntimeError(f"batch_feed: a field {tuple(a.shape)} {a.dtype} does not fit its static buffer {tuple(b.shape)} "
                               f"{b.dtype} (same row, same dtype, {n} samples, {batch} slots)")
        row = (a.numel() // max(n, 1)) * a.element_size()
        if row <= 0 or row % 4 or a.data_ptr() % 4 or b.data_ptr() % 4:
            raise RuntimeError(f"batch_feed: rows are copied as aligned 4-byte words; got a row of {row} bytes")
        if row > _lib.FEED_MAX_ROW_BYTES:
            raise RuntimeError(f"batch_feed: a row of {row} bytes is beyond PIT_FEED_MAX_ROW_BYTES ({_lib.FEED_MAX_ROW_BYTES})")
        rows.append(row)
    if state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous():
        raise RuntimeError("state must be 2 contiguous int64 values on the HIP device (new_feed_state)")
    if order is not None and (order.dtype != torch.int32 or order.numel() != n or not order.is_contiguous()):
        raise RuntimeError(f"order must be {n} contiguous int32 values on the HIP device")
    if indices is not None and (indices.dtype != torch.int32 or indices.numel() != batch or not indices.is_contiguous()):
        raise RuntimeError(f"indices must be {batch} contiguous int32 values on the HIP device")
    if n_valid is not None and (n_valid.dtype != torch.int32 or n_valid.numel() != 1):
        raise RuntimeError("n_valid must be one int32 value on the HIP device")
    if _capturing():
        _pin(*[o for o in src + dst + [state, order, indices, n_valid] if o is not None])
    k = len(src)
    src_a = (ctypes.c_void_p * k)(*[t.data_ptr() for t in src])
    dst_a = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dst])
    row_a = (ctypes.c_long * k)(*rows)
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 64):
        raise ValueError("seed must fit 64 bits")
    seed = seed - (1 << 64) if seed >= (1 << 63) else seed
    rc = _lib.lib().pit_batch_feed(ctypes.cast(src_a, ctypes.c_void_p), ctypes.cast(dst_a, ctypes.c_void_p),
                                   ctypes.cast(row_a, ctypes.c_void_p), k, n, batch, int(rank), int(world),
                                   1 if drop_last else 0, 1 if shuffle else 0, _lib.ptr(order), seed, state.data_ptr(),
                                   _lib.ptr(indices), _lib.ptr(n_valid), _lib.stream_ptr())
    _lib.check(rc, "pit_batch_feed")


@torch.compiler.disable
def batch_feed_points(src, dst, kinds, state: torch.Tensor, rank: int = 0, world: int = 1, drop_last: bool = True,
                      shuffle: bool = True, order=None, seed: int = 0, indices=None, n_valid=None, len_src=(None, None),
                      len_dst=(None, None), points=(None, None)) -> None:
    """One launch of pit_batch_feed_points (include/pit_hip.h): ``batch_feed`` that delivers, of every sample, a random subset
    of each cloud's points - the same subset for every field of a group, a function of (seed, epoch, sample, group) that
    ``engine.feed_points`` restates on the host.
      kinds       per field 0 (a whole row, as in ``batch_feed``), 1 or 2 (a point field of group 0 / 1): ``src[f]``
                  (n_samples, n_g, ...) against ``dst[f]`` (batch, m_g, ...) with m_g <= n_g, the same trailing shape and dtype; a
                  point is a whole number of 4-byte words
      len_src     per group, optional (n_samples,) int32: the real points of every sample's cloud (the rest is never read)
      len_dst     per group, optional (batch,) int32: receives min(m_g, length) per slot
      points      per group, optional (batch, m_g) int32: receives the source point of every destination point, -1 beyond
    Everything else as in ``batch_feed``."""
    src, dst, kinds = list(src), list(dst), [int(k) for k in kinds]
    if len(src) != len(dst) or len(src) != len(kinds) or not 1 <= len(src) <= _lib.FEED_MAX_FIELDS:
        raise ValueError(f"batch_feed_points takes 1..{_lib.FEED_MAX_FIELDS} fields, each with a source, a destination and a kind")
    len_src, len_dst, points = list(len_src), list(len_dst), list(points)
    if not len(len_src) == len(len_dst) == len(points) == 2:
        raise ValueError("batch_feed_points: len_src, len_dst and points hold one entry per group (two)")
    extra = [state, order, indices, n_valid] + len_src + len_dst + points
    for t in src + dst + extra:
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise RuntimeError("position_induced_transformer_amd: the data feed runs on the HIP device only; "
                               "got a CPU tensor (move the dataset and the step's buffers to 'cuda')")
    n, batch = src[0].shape[0], dst[0].shape[0]
    sizes, widths = [], [[0, 0], [0, 0]]                               # per group [n_g, m_g]
    for a, b, kind in zip(src, dst, kinds):
        if kind not in (_lib.FEED_WHOLE_ROW, _lib.FEED_POINTS_G0, _lib.FEED_POINTS_G1):
            raise ValueError(f"batch_feed_points: kind {kind} is none of 0 (whole row), 1, 2 (point field of group 0, 1)")
        if not a.is_contiguous() or not b.is_contiguous():
            raise RuntimeError("batch_feed_points: every field and every static buffer must be contiguous")
        lead = 1 if kind == _lib.FEED_WHOLE_ROW else 2
        if a.dtype != b.dtype or a.dim() < lead or b.dim() != a.dim() or a.shape[lead:] != b.shape[lead:] or a.shape[0] != n \
                or b.shape[0] != batch:
            raise RuntimeError(f"batch_feed_points: a field {tuple(a.shape)} {a.dtype} does not fit its static buffer "
                               f"{tuple(b.shape)} {b.dtype} ({n} samples, {batch} slots)")
        unit = a.element_size()
        for d in a.shape[lead:]:
            unit *= d
        if unit <= 0 or unit % 4 or a.data_ptr() % 4 or b.data_ptr() % 4:
            raise RuntimeError(f"batch_feed_points: rows and points are moved as aligned 4-byte words; got {unit} bytes")
        row = unit
        if lead == 2:
            g = kind - _lib.FEED_POINTS_G0
            if widths[g] != [0, 0] and widths[g] != [a.shape[1], b.shape[1]]:
                raise RuntimeError(f"batch_feed_points: the fields of group {g} disagree on the number of points "
                                   f"({widths[g]} and {[a.shape[1], b.shape[1]]})")
            widths[g] = [a.shape[1], b.shape[1]]
            if not 1 <= b.shape[1] <= a.shape[1]:
                raise RuntimeError(f"batch_feed_points: {b.shape[1]} destination points of {a.shape[1]} source points")
            row = unit * a.shape[1]
        if row > _lib.FEED_MAX_ROW_BYTES:
            raise RuntimeError(f"batch_feed_points: a sample's field of {row} bytes is beyond PIT_FEED_MAX_ROW_BYTES "
                               f"({_lib.FEED_MAX_ROW_BYTES})")
        sizes.append(unit)
    if state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous():
        raise RuntimeError("state must be 2 contiguous int64 values on the HIP device (new_feed_state)")
    if order is not None and (order.dtype != torch.int32 or order.numel() != n or not order.is_contiguous()):
        raise RuntimeError(f"order must be {n} contiguous int32 values on the HIP device")
    if indices is not None and (indices.dtype != torch.int32 or indices.numel() != batch or not indices.is_contiguous()):
        raise RuntimeError(f"indices must be {batch} contiguous int32 values on the HIP device")
    if n_valid is not None and (n_valid.dtype != torch.int32 or n_valid.numel() != 1):
        raise RuntimeError("n_valid must be one int32 value on the HIP device")
    for g in range(2):
        for what, t, count in (("len_src", len_src[g], n), ("len_dst", len_dst[g], batch), ("points", points[g], batch * widths[g][1])):
            if t is None:
                continue
            if widths[g] == [0, 0]:
                raise RuntimeError(f"batch_feed_points: {what}[{g}] without a point field of group {g}")
            if t.dtype != torch.int32 or t.numel() != count or not t.is_contiguous():
                raise RuntimeError(f"{what}[{g}] must be {count} contiguous int32 values on the HIP device")
    if _capturing():
        _pin(*[o for o in src + dst + extra if o is not None])
    k = len(src)
    src_a = (ctypes.c_void_p * k)(*[t.data_ptr() for t in src])
    dst_a = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dst])
    size_a = (ctypes.c_long * k)(*sizes)
    kind_a = (ctypes.c_int * k)(*kinds)
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 64):
        raise ValueError("seed must fit 64 bits")
    seed = seed - (1 << 64) if seed >= (1 << 63) else seed
    rc = _lib.lib().pit_batch_feed_points(ctypes.cast(src_a, ctypes.c_void_p), ctypes.cast(dst_a, ctypes.c_void_p),
                                          ctypes.cast(size_a, ctypes.c_void_p), ctypes.cast(kind_a, ctypes.c_void_p), k,
                                          widths[0][0], widths[0][1], widths[1][0], widths[1][1],
                                          _lib.ptr(len_src[0]), _lib.ptr(len_src[1]), _lib.ptr(len_dst[0]), _lib.ptr(len_dst[1]),
                                          _lib.ptr(points[0]), _lib.ptr(points[1]), n, batch, int(rank), int(world),
                                          1 if drop_last else 0, 1 if shuffle else 0, _lib.ptr(order), seed, state.data_ptr(),
                                          _lib.ptr(indices), _lib.ptr(n_valid), _lib.stream_ptr())
    _lib.check(rc, "pit_batch_feed_points")


FpsResult = collections.namedtuple("FpsResult", ("idx", "mesh", "lengths"))
FpsResult.__doc__ = """Result of ``farthest_point_sample``: ``idx`` (b, m) int32 - the picked points, -1 beyond a sample's picks;
``mesh`` (b, m, space_dim) fp32 - their coordinates (the cloud's bits), zeros beyond; ``lengths`` (b,) int32 - picks per sample,
min(m, length) - or None when the clouds had no lengths.  A batch-free (n, space_dim) cloud gives results without the batch axis."""


def fps_max_points(space_dim: int) -> int:
    """Largest cloud ``farthest_point_sample`` takes (the points live in registers): PIT_FPS_MAX_POINTS / _WIDE."""
    return _lib.FPS_MAX_POINTS if int(space_dim) <= 3 else _lib.FPS_MAX_POINTS_WIDE


def check_fps_shapes(mesh, n_samples, lengths=None, start=0) -> None:
    """Shape, dtype and envelope refusals of ``farthest_point_sample``, raised before the device check and before anything is
    launched."""
    _check_fps_shapes(mesh, n_samples, lengths, start, False)


def check_fps_large_shapes(mesh, n_samples, lengths=None, start=0, slice_points=0) -> None:
    """The same refusals for ``farthest_point_sample_large``: its own envelope, and ``slice_points``."""
    _check_fps_shapes(mesh, n_samples, lengths, start, True)
    if isinstance(slice_points, bool) or not isinstance(slice_points, (int, np.integer)) or \
            not (slice_points == 0 or (256 <= slice_points <= 65536 and slice_points % 256 == 0)):
        raise ValueError(f"slice_points must be 0 (the library's choice) or a multiple of 256 in [256, 65536], got {slice_points!r}")


def _check_fps_shapes(mesh, n_samples, lengths, start, large: bool) -> None:
    if not torch.is_tensor(mesh) or mesh.dim() not in (2, 3):
        raise ValueError("mesh must be a (b, n, space_dim) or (n, space_dim) tensor of point clouds")
    if mesh.dtype != torch.float32:
        raise ValueError(f"mesh must be fp32, got {mesh.dtype}")
    if 0 in mesh.shape:
        raise ValueError(f"the mesh has an empty axis: {tuple(mesh.shape)}")
    n, sdim = mesh.shape[-2], mesh.shape[-1]
    batch = mesh.shape[0] if mesh.dim() == 3 else 1
    if sdim > MAX_SPACE_DIM:
        raise ValueError(f"space_dim {sdim} beyond {MAX_SPACE_DIM} coordinates")
    if large and n > _lib.FPS_LARGE_MAX_POINTS:
        raise ValueError(f"a cloud of {n} points is beyond the large sampler's {_lib.FPS_LARGE_MAX_POINTS} points")
    if not large and n > fps_max_points(sdim):
        raise ValueError(f"a cloud of {n} points with {sdim} coordinates is beyond the sampler's {fps_max_points(sdim)} points "
                         f"(space_dim 1..3: {_lib.FPS_MAX_POINTS}, 4..8: {_lib.FPS_MAX_POINTS_WIDE})")
    if batch > 65535:
        raise ValueError(f"a batch of {batch} clouds is beyond 65535")
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or not 1 <= int(n_samples) <= n:
        raise ValueError(f"n_samples must be an integer in [1, {n}] (the padded width), got {n_samples!r}")
    if large and int(n_samples) > _lib.FPS_LARGE_MAX_SAMPLES:
        raise ValueError(f"n_samples {n_samples} is beyond the large sampler's {_lib.FPS_LARGE_MAX_SAMPLES} picks")
    for name, t in (("lengths", lengths), ("start", start)):
        if torch.is_tensor(t):
            if t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{name} must be an int32 or int64 tensor, got {t.dtype}")
            if t.numel() != batch:
                raise ValueError(f"{name} must hold one entry per sample: {t.numel()} entries for a batch of {batch}")
        elif name == "lengths" and t is not None and len(t) != batch:
            raise ValueError(f"lengths must hold one entry per sample: {len(t)} entries for a batch of {batch}")
    if not torch.is_tensor(start) and (isinstance(start, bool) or not isinstance(start, (int, np.integer))):
        raise ValueError(f"start must be an integer or a per-sample integer tensor, got {start!r}")


@torch.compiler.disable
def farthest_point_sample(mesh: torch.Tensor, n_samples: int, lengths=None, start=0) -> FpsResult:
    """One launch of pit_fps (include/pit_hip.h): ``n_samples`` points of every cloud by farthest-point sampling - from
    ``start``, repeatedly the point farthest (squared Euclidean distance, fp32) from everything picked so far, the lowest index
    among equals.  No host synchronisation, capturable; the same input gives the same bits.
      mesh       (b, n, space_dim) fp32 clouds, or (n, space_dim) for one cloud (results then drop the batch axis);
                 space_dim 1..3 with n <= 16384, 4..8 with n <= 4096
      lengths    real points per cloud (``as_lengths``: a device int32 tensor is used as it is, so a captured graph sees in-place
                 updates); rows beyond are never read.  A cloud shorter than ``n_samples`` gives ``lengths[s]`` picks.
      start      the first pick: an int, or a per-sample int tensor; clamped into the cloud
    Nothing differentiates through the choice: the result carries no autograd graph (gather ``mesh`` by ``idx`` for that)."""
    check_fps_shapes(mesh, n_samples, lengths, start)
    return _fps_run(mesh, n_samples, lengths, start, None)


@torch.compiler.disable
def farthest_point_sample_large(mesh: torch.Tensor, n_samples: int, lengths=None, start=0, slice_points: int = 0) -> FpsResult:
    """pit_fps_large (include/pit_hip.h): ``farthest_point_sample`` - the same arguments, the same result bit for bit - for
    clouds up to 4194304 points of 1..8 coordinates and up to 16384 picks.  The points stay in memory; a cloud is cut into slices
    of ``slice_points`` points, one workgroup each, and every pick is one launch (``n_samples`` dependent launches of one kernel),
    so the whole chip works on one cloud.  No host synchronisation, capturable; no atomics: the same input gives the same bits.
      slice_points   0: the library's choice (at most 256 slices per cloud); otherwise a multiple of 256 in [256, 65536].  The
                     result does not depend on it.
    The workspace (running distances and per-slice candidates) is allocated per call.  Small clouds are accepted too; there
    ``farthest_point_sample`` is one launch and faster."""
    check_fps_large_shapes(mesh, n_samples, lengths, start, slice_points)
    return _fps_run(mesh, n_samples, lengths, start, int(slice_points))


def _fps_run(mesh, n_samples, lengths, start, slice_points) -> FpsResult:
    """The launch of pit_fps (``slice_points`` None) or pit_fps_large, after the shape checks."""
    if not mesh.is_cuda:
        raise RuntimeError("position_induced_transformer_amd: the PiT hot path runs on the HIP device only; "
                           "got a CPU tensor (move the model and its inputs to 'cuda')")
    single = mesh.dim() == 2
    src = (mesh.unsqueeze(0) if single else mesh).detach()
    b, n, sdim = src.shape
    m = int(n_samples)
    if src.stride(2) != 1 or src.stride(1) != sdim or (b > 1 and src.stride(0) < n * sdim):
        src = src.contiguous()
    bstride = src.stride(0) if b > 1 else n * sdim
    len_t = None if lengths is None else as_lengths(lengths, src.device, b)
    start_t, start_all = None, 0
    if torch.is_tensor(start):
        start_t = start.detach().reshape(-1)
        if start_t.dtype != torch.int32 or start_t.device != src.device or not start_t.is_contiguous():
            start_t = start_t.to(device=src.device, dtype=torch.int32).contiguous()
    else:
        start_all = int(min(max(int(start), 0), n - 1))
    idx = torch.empty((b, m), device=src.device, dtype=torch.int32)
    out = torch.empty((b, m, sdim), device=src.device, dtype=torch.float32)
    out_len = None if len_t is None else torch.empty((b,), device=src.device, dtype=torch.int32)
    work = None
    if slice_points is not None:
        work = torch.empty((_lib.lib().pit_fps_large_workspace(b, n, slice_points),), device=src.device, dtype=torch.uint8)
    if _capturing():
        _pin(*[o for o in (src, len_t, start_t, work) if o is not None])
    if work is None:
        rc = _lib.lib().pit_fps(src.data_ptr(), b, n, sdim, bstride, _lib.ptr(len_t), _lib.ptr(start_t), start_all, m,
                                idx.data_ptr(), out.data_ptr(), _lib.ptr(out_len), _lib.stream_ptr())
        _lib.check(rc, "pit_fps")
    else:
        rc = _lib.lib().pit_fps_large(src.data_ptr(), b, n, sdim, bstride, _lib.ptr(len_t), _lib.ptr(start_t), start_all, m,
                                      idx.data_ptr(), out.data_ptr(), _lib.ptr(out_len), slice_points, work.data_ptr(),
                                      _lib.stream_ptr())
        _lib.check(rc, "pit_fps_large")
    if single:
        return FpsResult(idx[0], out[0], None if out_len is None else out_len[0])
    return FpsResult(idx, out, out_len)


KnnResult = collections.namedtuple("KnnResult", ("idx", "dist", "next"))
KnnResult.__doc__ = """Result of ``knn_box`` / ``knn_rows``: ``idx`` (.., N, k) int32 - the k nearest keys of every row, ascending
by (distance, key index); ``dist`` (.., N, k) fp32 - their distances, the kernel's own values; ``next`` (.., N) fp32 - the distance
of pair k + 1, +inf when k == J."""


def _check_knn_k(k, n_out: int, n_in: int, batch: int) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= n_in:
        raise ValueError(f"k must be an integer in [1, {n_in}] (the keys of a row), got {k!r}")
    if int(k) > KNN_MAX_K:
        raise ValueError(f"k = {k}: at most {KNN_MAX_K} neighbours are supported (the width the list layers accept)")
    if batch * n_out * int(k) >= 2 ** 31:
        raise ValueError(f"batch * N * k = {batch * n_out * int(k)} does not fit 31 bits")
    return int(k)


def _knn_periods(periods, sdim: int):
    """``periods`` as ``sdim`` Python floats, 0.0 for an axis that does not wrap; None when no axis wraps."""
    if periods is None:
        return None
    if torch.is_tensor(periods) or isinstance(periods, (str, bytes)) or not hasattr(periods, "__len__"):
        raise ValueError(f"periods must be None or a sequence of {sdim} entries, each a float or None, got {periods!r}")
    if len(periods) != sdim:
        raise ValueError(f"periods has {len(periods)} entries for meshes with {sdim} coordinates")
    out = []
    for p in periods:
        if p is None:
            out.append(0.0)
        elif isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)):
            raise ValueError(f"a period must be a float or None (a tensor period is not supported by the box kernel), got {p!r}")
        elif not math.isfinite(float(p)):
            raise ValueError(f"a period must be finite, got {p!r}")
        else:
            out.append(float(p) if float(p) > 0.0 else 0.0)
    return out if any(p > 0.0 for p in out) else None


def check_knn_box_shapes(mesh_out, mesh_in, k, periods=None):
    """Shape, dtype and envelope refusals of ``knn_box``, raised before the device check and before anything is launched.
    Returns (batch, n_out, n_in, space_dim, k, periods as floats or None)."""
    for name, t in (("mesh_out", mesh_out), ("mesh_in", mesh_in)):
        if not torch.is_tensor(t) or t.dim() not in (2, 3):
            raise ValueError(f"{name} must be a (n, space_dim) or (b, n, space_dim) tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be fp32, got {t.dtype}")
        if 0 in t.shape:
            raise ValueError(f"{name} has an empty axis: {tuple(t.shape)}")
    sdim = int(mesh_out.shape[-1])
    if int(mesh_in.shape[-1]) != sdim:
        raise ValueError(f"the meshes have {sdim} and {int(mesh_in.shape[-1])} coordinates")
    if sdim > MAX_SPACE_DIM:
        raise ValueError(f"space_dim {sdim} beyond {MAX_SPACE_DIM} coordinates")
    if mesh_out.dim() == 3 and mesh_in.dim() == 3 and mesh_out.shape[0] != mesh_in.shape[0]:
        raise ValueError(f"mesh_out holds {mesh_out.shape[0]} samples, mesh_in {mesh_in.shape[0]}")
    batch = int(mesh_out.shape[0]) if mesh_out.dim() == 3 else (int(mesh_in.shape[0]) if mesh_in.dim() == 3 else 1)
    n_out, n_in = int(mesh_out.shape[-2]), int(mesh_in.shape[-2])
    k = _check_knn_k(k, n_out, n_in, batch)
    return batch, n_out, n_in, sdim, k, _knn_periods(periods, sdim)


def check_knn_lengths(mesh_out, mesh_in, len_out, len_in) -> None:
    """What lengths on ``knn_box`` do not cover, refused before the device check: a length belongs to a per-sample (b, n, s) side
    (the rule of ``check_mixed``), one entry per sample."""
    batch = int(mesh_out.shape[0]) if mesh_out.dim() == 3 else (int(mesh_in.shape[0]) if mesh_in.dim() == 3 else 1)
    for name, given, mesh in (("len_out", len_out, mesh_out), ("len_in", len_in, mesh_in)):
        if given is None:
            continue
        if mesh.dim() != 3:
            raise ValueError(f"{name} for a mesh shared by the batch: every one of its points is real for every sample - lengths "
                             "belong to the per-sample side only")
        if torch.is_tensor(given) and given.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be an int32 or int64 tensor, got {given.dtype}")
        count = given.numel() if torch.is_tensor(given) else len(given)
        if count != batch:
            raise ValueError(f"{name} must hold one entry per sample: {count} entries for a batch of {batch}")


def check_knn_rows_shapes(m, k):
    """The same for ``knn_rows``.  Returns (batch, n_out, n_in, k)."""
    if not torch.is_tensor(m) or m.dim() not in (2, 3):
        raise ValueError("m must be a (N, J) or (b, N, J) tensor of distances")
    if m.dtype != torch.float32:
        raise ValueError(f"m must be fp32, got {m.dtype}")
    if 0 in m.shape:
        raise ValueError(f"m has an empty axis: {tuple(m.shape)}")
    batch = int(m.shape[0]) if m.dim() == 3 else 1
    n_out, n_in = int(m.shape[-2]), int(m.shape[-1])
    return batch, n_out, n_in, _check_knn_k(k, n_out, n_in, batch)


def _knn_need_gpu(*tensors) -> None:
    _need_gpu(*tensors)
    if len({t.device for t in tensors}) > 1:
        raise ValueError(f"the tensors live on different devices: {[str(t.device) for t in tensors]}")


def _knn_mesh(mesh, batch: int):
    """A mesh as the kernel reads it: (tensor to keep alive, sample stride in points).  A batch-free mesh, an expanded one and a
    batch of one are read in place with stride 0."""
    t = mesh.detach()
    n, sdim = int(t.shape[-2]), int(t.shape[-1])
    if t.dim() == 2 or batch == 1 or t.stride(0) == 0:
        rows = t if t.dim() == 2 else t[0]
        if rows.stride(1) != 1 or (n > 1 and rows.stride(0) != sdim):
            rows = rows.contiguous()
        return rows, 0
    if t.stride(2) != 1 or (n > 1 and t.stride(1) != sdim) or t.stride(0) % sdim or t.stride(0) < n * sdim:
        t = t.contiguous()
    return t, t.stride(0) // sdim


@torch.compiler.disable
def knn_box(mesh_out: torch.Tensor, mesh_in: torch.Tensor, k: int, periods=None, len_out=None, len_in=None) -> KnnResult:
    """One launch of pit_knn_box (include/pit_hip.h): for every point of ``mesh_out`` its ``k`` nearest points of ``mesh_in``
    under the squared distance of a box - Euclidean, or with ``periods[a]`` (a float; None: no wrap) the period of axis a, the op
    sequence of metric.sqdist_euclid / sqdist_periodic_box - ascending by (distance, key index), the lowest index among equals.
    The N x J matrix is never formed; no workspace, no host synchronisation, capturable; the same input gives the same bits.
      mesh_out   (N, s) or (b, N, s) fp32; mesh_in (J, s) or (b, J, s) fp32; a batch-free mesh is shared by the batch and read in place
      k          1 .. min(J, 2048)
    Results are (N, k) / (N,) when both meshes are batch-free, (b, N, k) / (b, N) otherwise.  Nothing differentiates through the
    choice (recompute the listed distances for that: metric.knn_lists_box).
      len_out / len_in   a RAGGED batch (pit_knn_box_ragged): the point counts of the per-sample sides (``as_lengths`` forms; a
                 shared mesh takes none), read on the device - no synchronisation, so a captured launch follows lengths
                 overwritten in place.  Sample s searches its first L = len_in[s] keys only (the rest may hold NaN) and a real
                 row equals ``knn_box`` on the trimmed sample with min(k, L) neighbours bit for bit; its further slots hold key
                 -1 / distance 0 and ``next`` is +inf when k >= L; rows >= len_out[s] hold -1 / 0 / +inf.  ``k`` is checked
                 against the padded width."""
    batch, n_out, n_in, sdim, k, per = check_knn_box_shapes(mesh_out, mesh_in, k, periods)
    check_knn_lengths(mesh_out, mesh_in, len_out, len_in)
    _knn_need_gpu(mesh_out, mesh_in)
    mo, so = _knn_mesh(mesh_out, batch)
    mi, si = _knn_mesh(mesh_in, batch)
    dev = mo.device
    idx = torch.empty((batch, n_out, k), device=dev, dtype=torch.int32)
    dist = torch.empty((batch, n_out, k), device=dev, dtype=torch.float32)
    nxt = torch.empty((batch, n_out), device=dev, dtype=torch.float32)
    per_c = None if per is None else (ctypes.c_float * sdim)(*per)
    per_p = None if per_c is None else ctypes.cast(per_c, ctypes.c_void_p)
    if len_out is not None or len_in is not None:
        lo = None if len_out is None else as_lengths(len_out, dev, batch)
        li = None if len_in is None else as_lengths(len_in, dev, batch)
        if _capturing():
            _pin(mo, mi, lo, li)
        rc = _lib.lib().pit_knn_box_ragged(mo.data_ptr(), mi.data_ptr(), batch, n_out, n_in, sdim, so, si, per_p, k, _lib.ptr(lo),
                                           _lib.ptr(li), idx.data_ptr(), dist.data_ptr(), nxt.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_knn_box_ragged")
        return KnnResult(idx, dist, nxt)
    if _capturing():
        _pin(mo, mi)
    rc = _lib.lib().pit_knn_box(mo.data_ptr(), mi.data_ptr(), batch, n_out, n_in, sdim, so, si, per_p, k, idx.data_ptr(),
                                dist.data_ptr(), nxt.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "pit_knn_box")
    if mesh_out.dim() == 2 and mesh_in.dim() == 2:
        return KnnResult(idx[0], dist[0], nxt[0])
    return KnnResult(idx, dist, nxt)


@torch.compiler.disable
def knn_rows(m: torch.Tensor, k: int) -> KnnResult:
    """One launch of pit_knn_rows: the ``k`` smallest entries of every row of ``m`` - (N, J) or (b, N, J) fp32 distances under ANY
    metric, finite and >= 0 (not checked) - ascending by (value, column), the lowest column among equals: torch.sort(stable=True)
    cut at k.  A view with a leading dimension beyond J is read in place (its guard columns are never read)."""
    batch, n_out, n_in, k = check_knn_rows_shapes(m, k)
    _knn_need_gpu(m)
    src = m.detach()
    if src.stride(-1) != 1 or (n_out > 1 and src.stride(-2) < n_in):
        src = src.contiguous()
    ld = src.stride(-2) if n_out > 1 else n_in
    bstride = 0
    if src.dim() == 3 and batch > 1 and src.stride(0) != 0:
        if src.stride(0) < (n_out - 1) * ld + n_in:
            src = src.contiguous()
            ld = n_in
        bstride = src.stride(0)
    idx = torch.empty((batch, n_out, k), device=src.device, dtype=torch.int32)
    dist = torch.empty((batch, n_out, k), device=src.device, dtype=torch.float32)
    nxt = torch.empty((batch, n_out), device=src.device, dtype=torch.float32)
    if _capturing():
        _pin(src)
    rc = _lib.lib().pit_knn_rows(src.data_ptr(), ld, bstride, batch, n_out, n_in, k, idx.data_ptr(), dist.data_ptr(),
                                 nxt.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "pit_knn_rows")
    if m.dim() == 2:
        return KnnResult(idx[0], dist[0], nxt[0])
    return KnnResult(idx, dist, nxt)


def knn_last_form() -> int:
    """pit_knn_last_form: 1 (the row's distances in registers) or 2 (streamed) for this process's latest knn launch, 0 before."""
    return int(_lib.lib().pit_knn_last_form())


def knn_box_restated(mesh_out, mesh_in, k: int, periods=None, row_chunk: int = 512, len_out=None, len_in=None) -> KnnResult:
    """``knn_box`` restated on the host in numpy fp32, operation by operation (the loop of include/pit_hip.h): t = |x - y|,
    u = minimum(t, p - t) on a wrapped axis, d = ((u0*u0 + u1*u1) + u2*u2) + ..., a stable ascending sort of every row, cut at
    ``k``.  CPU tensors in, CPU tensors out, the shapes and dtypes of ``knn_box``; for tests.  ``len_out`` / ``len_in``: the
    ragged form of ``knn_box`` - every sample restated on its first len_in[s] keys and len_out[s] rows, the rest filled with
    -1 / 0 / +inf."""
    batch, n_out, n_in, sdim, k, per = check_knn_box_shapes(mesh_out, mesh_in, k, periods)
    check_knn_lengths(mesh_out, mesh_in, len_out, len_in)
    ragged = len_out is not None or len_in is not None
    lens = [None if v is None else [max(1, min(int(x), w)) for x in (v.tolist() if torch.is_tensor(v) else v)]
            for v, w in ((len_out, n_out), (len_in, n_in))]
    mo = mesh_out.detach().cpu().numpy().astype(np.float32, copy=False)
    mi = mesh_in.detach().cpu().numpy().astype(np.float32, copy=False)
    idx = np.full((batch, n_out, k), -1, np.int32)
    dist = np.zeros((batch, n_out, k), np.float32)
    nxt = np.full((batch, n_out), np.inf, np.float32)
    k_all = k
    for s in range(batch):
        x_all, y = (mo[s] if mo.ndim == 3 else mo), (mi[s] if mi.ndim == 3 else mi)
        lo, n_in = (n_out if lens[0] is None else lens[0][s]), (int(mesh_in.shape[-2]) if lens[1] is None else lens[1][s])
        x_all, y, k = x_all[:lo], y[:n_in], min(k_all, n_in)
        for r0 in range(0, lo, int(row_chunk)):
            x = x_all[r0:r0 + int(row_chunk)]
            d = None
            for a in range(sdim):
                t = np.abs(x[:, None, a] - y[None, :, a])
                if per is not None and per[a] > 0.0:
                    t = np.minimum(t, np.float32(per[a]) - t)
                q = t * t
                d = q if d is None else d + q
            assert d.dtype == np.float32
            order = np.argsort(d, axis=-1, kind="stable")
            srt = np.take_along_axis(d, order, axis=-1)
            idx[s, r0:r0 + len(x), :k] = order[:, :k]
            dist[s, r0:r0 + len(x), :k] = srt[:, :k]
            nxt[s, r0:r0 + len(x)] = srt[:, k] if k < n_in else np.float32(np.inf)
    out = KnnResult(torch.from_numpy(idx), torch.from_numpy(dist), torch.from_numpy(nxt))
    if mesh_out.dim() == 2 and mesh_in.dim() == 2 and not ragged:
        return KnnResult(out.idx[0], out.dist[0], out.next[0])
    return out


GeoResult = collections.namedtuple("GeoResult", ("idx", "dist", "next", "status"))
GeoResult.__doc__ = """Result of ``geo_knn``: ``idx`` (.., N, k) int32 - the keys of every row's k nearest reachable key vertices,
ascending by (path length, vertex index), -1 in the slots a row does not fill; ``dist`` (.., N, k) fp32 - their path lengths (not
squared), 0 in unfilled slots; ``next`` (.., N) fp32 - a lower bound of the length of the nearest key the list leaves out (exact
when every vertex is a key), +inf when there is none and on padded and truncated rows; ``status`` (.., N) int32 - 1 where the
search met its ``reach`` budget (the row lists the keys settled until then, exactly), else 0."""
GEO_MAX_K = _lib.GEO_MAX_K
GEO_MAX_REACH = _lib.GEO_MAX_REACH


def geo_default_reach(k: int) -> int:
    """The ``reach`` ``geo_knn`` takes when none is given: the power of two >= 8 k, at most 4096 (and never below k)."""
    r = 1
    while r < 8 * int(k):
        r *= 2
    return max(int(k), min(GEO_MAX_REACH, r))


def check_geo_shapes(adj, w, k, sources=None, key_of=None, len_v=None, reach=None):
    """Shape, dtype and envelope refusals of ``geo_knn``, raised before the device check and before anything is launched.
    Returns (batch, n_vert, n_edge, n_rows, k, reach, batched): ``batched`` says whether the results carry a batch axis."""
    for name, t, dt in (("adj", adj, torch.int32), ("w", w, torch.float32)):
        if not torch.is_tensor(t) or t.dim() not in (2, 3):
            raise ValueError(f"{name} must be a (V, G) or (b, V, G) tensor")
        if t.dtype != dt:
            raise ValueError(f"{name} must be {dt}, got {t.dtype}")
        if 0 in t.shape:
            raise ValueError(f"{name} has an empty axis: {tuple(t.shape)}")
    if tuple(adj.shape) != tuple(w.shape):
        raise ValueError(f"adj {tuple(adj.shape)} and w {tuple(w.shape)} must have one shape")
    n_vert, n_edge = int(adj.shape[-2]), int(adj.shape[-1])
    if n_vert * n_edge >= 2 ** 31:
        raise ValueError(f"V * G = {n_vert * n_edge} does not fit 31 bits")
    batches = {"adj": int(adj.shape[0])} if adj.dim() == 3 else {}
    for name, t, width in (("sources", sources, None), ("key_of", key_of, n_vert)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() not in (1, 2):
            raise ValueError(f"{name} must be None or a ({'N' if width is None else 'V'},) or (b, {'N' if width is None else 'V'}) tensor")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, got {t.dtype}")
        if 0 in t.shape:
            raise ValueError(f"{name} has an empty axis: {tuple(t.shape)}")
        if width is not None and int(t.shape[-1]) != width:
            raise ValueError(f"{name} has {int(t.shape[-1])} entries for a graph on {width} vertices")
        if t.dim() == 2:
            batches[name] = int(t.shape[0])
    if len(set(batches.values())) > 1:
        raise ValueError(f"the batched arguments hold different numbers of samples: {batches}")
    batch = next(iter(batches.values())) if batches else 1
    if len_v is not None:
        if torch.is_tensor(len_v) and len_v.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"len_v must be an int32 or int64 tensor, got {len_v.dtype}")
        count = len_v.numel() if torch.is_tensor(len_v) else len(len_v)
        if count != batch:
            raise ValueError(f"len_v must hold one entry per sample: {count} entries for a batch of {batch}")
    n_rows = n_vert if sources is None else int(sources.shape[-1])
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError(f"k must be a positive integer, got {k!r}")
    k = int(k)
    if k > GEO_MAX_K:
        raise ValueError(f"k = {k}: at most {GEO_MAX_K} neighbours are supported by the geodesic builder")
    if reach is None:
        reach = geo_default_reach(k)
    if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)):
        raise ValueError(f"reach must be None or an integer, got {reach!r}")
    reach = int(reach)
    if not k <= reach <= GEO_MAX_REACH:
        raise ValueError(f"reach = {reach}: the discovered vertices of a row are bounded by k = {k} <= reach <= {GEO_MAX_REACH}")
    if batch * n_rows * k >= 2 ** 31:
        raise ValueError(f"batch * N * k = {batch * n_rows * k} does not fit 31 bits")
    return batch, n_vert, n_edge, n_rows, k, reach, bool(batches) or len_v is not None


def _geo_shared(t, batch: int, width: int):
    """An argument of ``geo_knn`` as the kernel reads it: (contiguous tensor to keep alive, sample stride in elements, 0 = shared)."""
    t = t.detach()
    lead = t.dim() - (1 if width is None else 2)          # 1: a batch axis
    if lead == 0 or batch == 1 or t.stride(0) == 0:
        rows = t if lead == 0 else t[0]
        return rows.contiguous(), 0
    t = t.contiguous()
    return t, t.stride(0)


@torch.compiler.disable
def geo_knn(adj: torch.Tensor, w: torch.Tensor, k: int, sources=None, key_of=None, len_v=None, reach=None) -> GeoResult:
    """One launch of pit_geo_knn (include/pit_hip.h): for every row its ``k`` nearest key vertices under the PATH LENGTH of a
    graph - a truncated single-source shortest-path search per row - ascending by (length, vertex index), the lowest vertex index
    among equals, in the list layers' format.  No workspace, no host synchronisation, capturable; the same input gives the same bits.
      adj, w     (V, G) or (b, V, G) int32 / fp32, padded adjacency: edge t of vertex u leads to adj[u, t] and has length w[u, t];
                 valid iff 0 <= adj[u, t] < Vs.  Directed; self edges and duplicates are harmless.  Weights finite and >= 0 (not
                 checked; nothing is addressed out of bounds whatever they hold).  The length of a path is summed in fp32 along it,
                 one rounded add per edge; D(v) is the least such sum.
      sources    (N,) or (b, N) int32: the start vertex of every row; None: every vertex, N = V.  A source outside [0, Vs) is a
                 padded row (-1 / 0 / +inf / 0).
      key_of     (V,) or (b, V) int32: a vertex's key index, < 0 = no key; None: the identity
      len_v      the vertices of every sample (``as_lengths`` forms), read on the device: Vs = len_v[s] clamped into [1, V];
                 adjacency rows of vertices >= Vs are never read
      k          1 .. 1024;  reach: k .. 4096, None: the power of two >= 8 k (at most 4096) - the bound on the vertices a row
                 discovers (settled or in its frontier); a row that would discover more stops with status 1 and lists the keys it
                 has settled, whose lengths are exact.  Truncation is reported, never silent.
    Results carry a batch axis when an argument does or ``len_v`` is given.  Nothing differentiates through the search."""
    batch, n_vert, n_edge, n_rows, k, reach, batched = check_geo_shapes(adj, w, k, sources, key_of, len_v, reach)
    _need_gpu(w)
    given = [t for t in (adj, w, sources, key_of) if t is not None]
    if not all(t.is_cuda for t in given):
        raise RuntimeError("position_induced_transformer_amd: geo_knn runs on the HIP device only; got a CPU tensor")
    if len({t.device for t in given}) > 1:
        raise ValueError(f"the tensors live on different devices: {[str(t.device) for t in given]}")
    dev = w.device
    adj_t, adj_s = _geo_shared(adj, batch, n_edge)
    w_t, w_s = _geo_shared(w, batch, n_edge)
    if adj_s != w_s:                                      # (one of the two expanded, the other not: one stride serves both)
        adj_t, w_t = adj.detach().expand(batch, -1, -1).contiguous(), w.detach().expand(batch, -1, -1).contiguous()
        adj_s = n_vert * n_edge
    src_t, src_s = (None, 0) if sources is None else _geo_shared(sources, batch, None)
    key_t, key_s = (None, 0) if key_of is None else _geo_shared(key_of, batch, None)
    len_t = None if len_v is None else as_lengths(len_v, dev, batch)
    idx = torch.empty((batch, n_rows, k), device=dev, dtype=torch.int32)
    dist = torch.empty((batch, n_rows, k), device=dev, dtype=torch.float32)
    nxt = torch.empty((batch, n_rows), device=dev, dtype=torch.float32)
    status = torch.empty((batch, n_rows), device=dev, dtype=torch.int32)
    if _capturing():
        _pin(adj_t, w_t, src_t, key_t, len_t)
    rc = _lib.lib().pit_geo_knn(adj_t.data_ptr(), w_t.data_ptr(), adj_s, batch, n_vert, n_edge, _lib.ptr(src_t), src_s, n_rows,
                                _lib.ptr(key_t), key_s, _lib.ptr(len_t), k, reach, idx.data_ptr(), dist.data_ptr(), nxt.data_ptr(),
                                status.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "pit_geo_knn")
    if not batched:
        return GeoResult(idx[0], dist[0], nxt[0], status[0])
    return GeoResult(idx, dist, nxt, status)


def _geo_row_restated(adj, w, vs: int, src: int, key, k: int, reach: int):
    """One row of ``geo_knn_restated``: (keys, lengths, next, status) as Python lists / floats."""
    import heapq
    tent, settled, cands = {src: 0.0}, {}, []
    heap = [(0.0, src)]                                   # (tentative length, vertex): the order of the header
    kth, front, truncated = None, float("inf"), False
    while True:
        while heap and (heap[0][1] in settled or tent.get(heap[0][1]) != heap[0][0]):
            heapq.heappop(heap)                           # (an entry a shorter path has replaced)
        if not heap:
            break                                         # the frontier is empty
        d_v, v = heap[0]
        if len(cands) >= k and d_v > kth:
            front = d_v                                   # complete: nothing the frontier holds can enter the list
            break
        heapq.heappop(heap)
        settled[v] = d_v
        del tent[v]
        if key is None or key[v] >= 0:
            cands.append((d_v, v))
            if len(cands) == k:
                kth = d_v
        new_len = np.float32(d_v) + w[v]                  # fl32(D(u) + w(u, v)), one rounded add per edge
        assert new_len.dtype == np.float32
        row = adj[v]
        for t in range(row.shape[0]):
            a = int(row[t])
            if not 0 <= a < vs or a in settled:
                continue
            n = float(new_len[t]) + 0.0                   # (-0.0 counts as +0.0)
            old = tent.get(a)
            if old is None:
                if len(settled) + len(tent) >= reach:     # the discovered set would exceed the budget
                    truncated = True
                    break
                tent[a] = n
                heapq.heappush(heap, (n, a))
            elif n < old:
                tent[a] = n
                heapq.heappush(heap, (n, a))
        if truncated:
            break
    cands.sort()
    nxt = float("inf")
    if not truncated:
        nxt = min(front, cands[k][0]) if len(cands) > k else front
    cands = cands[:k]
    return [v if key is None else int(key[v]) for _, v in cands], [d for d, _ in cands], nxt, 1 if truncated else 0


def geo_knn_restated(adj, w, k: int, sources=None, key_of=None, len_v=None, reach=None) -> GeoResult:
    """``geo_knn`` restated on the host, step by step (the search of include/pit_hip.h): label-setting search in the order
    (tentative length, vertex index) with numpy fp32 adds, the completion test (k candidates settled and the frontier strictly
    beyond the k-th), the ``reach`` budget checked at every discovery, the settled key vertices sorted by (length, vertex) and
    cut at ``k``.  CPU tensors in, CPU tensors out, the shapes and dtypes of ``geo_knn``; for tests."""
    batch, n_vert, n_edge, n_rows, k, reach, batched = check_geo_shapes(adj, w, k, sources, key_of, len_v, reach)
    adj_n, w_n = adj.detach().cpu().numpy(), w.detach().cpu().numpy().astype(np.float32, copy=False)
    src_n = None if sources is None else sources.detach().cpu().numpy()
    key_n = None if key_of is None else key_of.detach().cpu().numpy()
    lens = None if len_v is None else [max(1, min(int(x), n_vert)) for x in (len_v.tolist() if torch.is_tensor(len_v) else len_v)]
    idx = np.full((batch, n_rows, k), -1, np.int32)
    dist = np.zeros((batch, n_rows, k), np.float32)
    nxt = np.full((batch, n_rows), np.inf, np.float32)
    status = np.zeros((batch, n_rows), np.int32)
    for s in range(batch):
        a_s, w_s = (adj_n[s] if adj_n.ndim == 3 else adj_n), (w_n[s] if w_n.ndim == 3 else w_n)
        key = None if key_n is None else (key_n[s] if key_n.ndim == 2 else key_n)
        vs = n_vert if lens is None else lens[s]
        for i in range(n_rows):
            src = i if src_n is None else int(src_n[s, i] if src_n.ndim == 2 else src_n[i])
            if not 0 <= src < vs:
                continue
            keys, lengths, nx, st = _geo_row_restated(a_s, w_s, vs, src, key, k, reach)
            idx[s, i, :len(keys)] = keys
            dist[s, i, :len(keys)] = lengths
            nxt[s, i], status[s, i] = nx, st
    out = GeoResult(torch.from_numpy(idx), torch.from_numpy(dist), torch.from_numpy(nxt), torch.from_numpy(status))
    if not batched:
        return GeoResult(out.idx[0], out.dist[0], out.next[0], out.status[0])
    return out


class _InstanceNorm(torch.autograd.Function):
    """nn.InstanceNorm1d over the point axis on the (batch, points, channels) layout
    (train_vorticity.py:43,56,59), no permutes."""

    @staticmethod
    def forward(ctx, x, eps: float):
        _need_gpu(x)
        x = _row_view(x)
        b, npts, nch = x.shape
        y = torch.empty((b, npts, nch), device=x.device, dtype=torch.float32)
        rstd = torch.empty((b, nch), device=x.device, dtype=torch.float32)
        rc = _lib.lib().pit_instance_norm_fwd(x.data_ptr(), x.stride(1), x.stride(0), b, npts, nch, float(eps),
                                              y.data_ptr(), rstd.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_instance_norm_fwd")
        ctx.save_for_backward(y, rstd)
        return y

    @staticmethod
    def backward(ctx, d_y):
        y, rstd = ctx.saved_tensors
        b, npts, nch = y.shape
        d_y = d_y.contiguous()
        d_x = torch.empty_like(y)
        rc = _lib.lib().pit_instance_norm_bwd(d_y.data_ptr(), y.data_ptr(), rstd.data_ptr(), b, npts, nch,
                                              d_x.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_instance_norm_bwd")
        return d_x, None


@torch.compiler.disable
def instance_norm_points(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """(x - mean over points) / sqrt(var over points + eps) per (sample, channel) of a (b, L, C) tensor."""
    return _InstanceNorm.apply(x, eps)


_MATH = threading.local()


def _math_code() -> int:
    return MATH_MODES[getattr(_MATH, "mode", "fp32")]


def set_math_mode(mode: str) -> None:
    """'fp32' (default, the reference's arithmetic) or 'bf16' (bf16 MFMA operands, fp32 accumulate) for
    the attention / MLP contractions (the small-regime fused MLP kernels contract in fp32 in both modes - they
    are latency-bound - and the fused processor blocks run in fp32 mode only: bf16 mode takes the per-layer path).
    In bf16 mode the decoder tail is also STORED as bf16 when its shape allows (BF16_STORAGE, pit.decoder).  Host-side, per Python thread: the mode is an ARGUMENT of every
    C-ABI call (the library keeps no mode of its own), read when an operator's forward runs and reused
    by its backward; a captured hipGraph keeps the mode its launches were captured with."""
    if mode not in MATH_MODES:
        raise ValueError(f"math mode must be one of {sorted(MATH_MODES)}, got {mode!r}")
    _MATH.mode = mode


def get_math_mode() -> str:
    return getattr(_MATH, "mode", "fp32")


class math_mode:
    """`with ops.math_mode('bf16'): ...` - scoped set_math_mode."""

    def __init__(self, mode: str):
        self.mode, self.prev = mode, None

    def __enter__(self):
        self.prev = get_math_mode()
        set_math_mode(self.mode)
        return self

    def __exit__(self, *exc):
        set_math_mode(self.prev)
        return False


# Reproducible mode: every gradient summed in a fixed order - the per-layer path (no fused launch, no
# rider), weight gradients through pit_mlp_bwd_params_ordered_mfma, d(values) of candidate-list layers from transposed lists
# whose ranges are sorted, overflowed rows added by pit_posatt_overflow_dv_ordered.  fp32 math mode only.  Per thread, like the
# math mode; PIT_REPRODUCIBLE=1 in the environment is the initial value (unmodified scripts).  Read in an operator's forward
# and remembered on its autograd context.  NOT tied to torch.use_deterministic_algorithms.
_REPRO = threading.local()
_DEFAULT_REPRO = os.environ.get("PIT_REPRODUCIBLE", "0").strip().lower() not in ("", "0", "false", "off", "no")


def set_reproducible(on: bool) -> None:
    _REPRO.on = bool(on)


def get_reproducible() -> bool:
    return bool(getattr(_REPRO, "on", _DEFAULT_REPRO))


class reproducible:
    """`with ops.reproducible(): ...` - scoped set_reproducible (restored on exit, also after an exception)."""

    def __init__(self, on: bool = True):
        self.on, self.prev = bool(on), None

    def __enter__(self):
        self.prev = get_reproducible()
        set_reproducible(self.on)
        return self

    def __exit__(self, *exc):
        set_reproducible(self.prev)
        return False


def reproducible_wanted() -> bool:
    """get_reproducible(), refusing what the mode does not cover before anything is launched."""
    if not get_reproducible():
        return False
    if get_math_mode() != "fp32":
        raise NotImplementedError("the reproducible mode (ops.set_reproducible) runs in the fp32 math mode only: the bf16 mode's "
                                  "kernels add their partial sums in no fixed order")
    return True


def head_scale(lmda: torch.Tensor) -> torch.Tensor:
    """c = tan(0.25*pi*(1-1e-7)*(1+sin(lmda))) on device (pit.py:48)."""
    _need_gpu(lmda)
    flat = lmda.detach().reshape(-1).contiguous()
    out = torch.empty_like(flat)
    _lib.check(_lib.lib().pit_head_scale(flat.data_ptr(), flat.numel(), out.data_ptr(), _lib.stream_ptr()),
               "pit_head_scale")
    return out.reshape(lmda.shape)


def debug_mfma_tile(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """D = A(32x8) @ B(8x32) through the kernels' MFMA fragment maps (layout self-test)."""
    _need_gpu(a, b)
    d = torch.empty((32, 32), device=a.device, dtype=torch.float32)
    _lib.check(_lib.lib().pit_debug_mfma_tile(a.contiguous().data_ptr(), b.contiguous().data_ptr(), d.data_ptr(),
                                              _lib.stream_ptr()), "pit_debug_mfma_tile")
    return d


def gemm_launch_counts(reset: bool = False) -> list:
    """The calling thread's launch record of the GEMM core (pit_debug_gemm_counts): one slot per PIT_GEMM_* kind of
    include/pit_hip.h, in order (the library says how many).  Host-side integers; no device work."""
    fn = _lib.lib().pit_debug_gemm_counts
    n = fn(None, 0, 0)
    buf = (ctypes.c_int * n)()
    fn(buf, n, 1 if reset else 0)
    return list(buf)


def att_launch_counts(reset: bool = False) -> list:
    """The calling thread's launch record of the masked-layer dispatcher (pit_debug_att_counts): one slot per PIT_ATT_* kind of
    include/pit_hip.h, in order (the library says how many).  Host-side integers; no device work."""
    fn = _lib.lib().pit_debug_att_counts
    n = fn(None, 0, 0)
    buf = (ctypes.c_int * n)()
    fn(buf, n, 1 if reset else 0)
    return list(buf)


def dense_launch_counts(reset: bool = False) -> list:
    """The calling thread's launch record of the dense (MFMA) position-attention launchers (pit_debug_dense_counts): one slot
    per PIT_DENSE_* kind of include/pit_hip.h, in order (the library says how many).  Host-side integers; no device work."""
    fn = _lib.lib().pit_debug_dense_counts
    n = fn(None, 0, 0)
    buf = (ctypes.c_int * n)()
    fn(buf, n, 1 if reset else 0)
    return list(buf)


_ = ctypes  # keep the import explicit: pointers cross the ABI as plain integers
