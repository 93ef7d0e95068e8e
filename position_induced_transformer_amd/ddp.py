"""Batch-axis data parallelism for PiT: one process per GPU, one all-reduce per step.

The reference has no distributed code; the path shards on the batch axis,
every rank holds a full replica and the only exchange is the parameter-gradient sum.
All parameters' ``.grad`` are views into ONE flat fp32 buffer (79 k floats for Darcy,
1.27 M for Elasticity - a single sub-25 MB message), so a step issues exactly one
``all_reduce`` (RCCL over xGMI with backend "nccl"; gloo in the CPU tests).

``RelLpNorm`` SUMS over the batch (utils.py:98), so the single-process gradient of a
global batch equals the SUM of the per-rank gradients: the default reduction is SUM,
not DDP's mean (SURVEY section 8(e) loss-scaling note).
"""
from __future__ import annotations

import contextlib
from typing import Iterable, List, NamedTuple, Optional

import torch
import torch.distributed as dist


class FlatGradients:
    """Owns a flat gradient buffer and points every parameter's ``.grad`` into it.  With
    ``flatten_params=True`` the parameters themselves are also re-homed into one flat buffer
    (``flat_params``; values preserved), which is what the fused optimizer step works on."""

    def __init__(self, params: Iterable[torch.nn.Parameter], flatten_params: bool = False,
                 tail: Iterable[torch.nn.Parameter] = ()):
        """``tail``: parameters to lay out LAST, as one contiguous segment ``flat[tail_start:]`` - the bucket a
        two-bucket step all-reduces early (their gradients are complete before the backward pass ends, see
        engine.TrainStep(all_reduce_buckets=2))."""
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        tail_ids = {id(p) for p in tail}
        self.params = [p for p in self.params if id(p) not in tail_ids] + [p for p in self.params if id(p) in tail_ids]
        n_head_params = sum(1 for p in self.params if id(p) not in tail_ids)
        dev, dt = self.params[0].device, self.params[0].dtype
        # every parameter starts on a 64-byte boundary of the flat buffers (zero padding in between):
        # the GEMM kernels use 16-byte operand loads only on aligned weight matrices
        align = 16
        offsets, total = [], 0
        for p in self.params:
            offsets.append(total)
            total += (p.numel() + align - 1) // align * align
        self.flat = torch.zeros(total, device=dev, dtype=dt)
        self.flat_params = torch.zeros(total, device=dev, dtype=dt) if flatten_params else None
        self.offsets = offsets
        self.tail_start = offsets[n_head_params] if n_head_params < len(offsets) else total
        self._views = []
        for p, off in zip(self.params, offsets):
            n = p.numel()
            view = self.flat[off:off + n].view_as(p)
            self._views.append(view)
            p.grad = view
            if p.is_cuda:
                from . import ops
                ops.mark_inplace_grad(p, view)      # the backward kernels may accumulate into this view in place
            if flatten_params:
                self.flat_params[off:off + n].copy_(p.data.reshape(-1))
                p.data = self.flat_params[off:off + n].view_as(p)

    last_work = None          # Work handle of the last eager (not captured) all-reduce on a device backend

    def zero_(self) -> None:
        """Clear the gradients and keep them attached.  Use this (or ``zero_grad(set_to_none=False)``)
        instead of ``optimizer.zero_grad()``, whose default ``set_to_none=True`` drops the views; if
        a loop does call it, :meth:`attach` (run by ``all_reduce`` / ``FlatAdam.step``) repairs it."""
        self.attach(keep_values=False)
        self.flat.zero_()

    def attach(self, keep_values: bool = True) -> int:
        """Make every parameter's ``.grad`` the registered view into the flat buffer again.

        ``optimizer.zero_grad()`` (train_darcy.py:127; ``set_to_none=True`` by default) sets ``.grad``
        to None, after which autograd allocates fresh gradient tensors OUTSIDE the flat buffer and a
        flat all-reduce would sum stale memory.  For each detached parameter the current gradient
        (if any and ``keep_values``) is copied into its slot - a missing gradient zeroes the slot -
        and ``.grad`` points at the slot again.  Returns the number of parameters re-attached."""
        fixed = 0
        for p, view in zip(self.params, self._views):
            g = p.grad
            if g is not None and g.data_ptr() == view.data_ptr() and g.shape == view.shape:
                continue
            if g is not None and keep_values:
                view.copy_(g.detach().reshape(view.shape))
            else:
                view.zero_()
            p.grad = view
            fixed += 1
        return fixed

    def dense(self) -> torch.Tensor:
        """The gradients concatenated in parameter order WITHOUT the alignment padding (a copy)."""
        return torch.cat([p.grad.reshape(-1) for p in self.params])

    def all_reduce(self, average: bool = False, group=None, part: str = "all") -> None:
        """Sum (or average) the flat buffer over the ranks; no-op without a process group.  ``part``: "all", or one
        of the two buckets of a two-bucket step - "tail" (``flat[tail_start:]``) / "head" (``flat[:tail_start]``)."""
        if part not in ("all", "head", "tail"):
            raise ValueError(f"part must be 'all', 'head' or 'tail', got {part!r}")
        if part != "tail":
            self.attach()                   # .grad tensors that left the flat buffer are copied back first
        if not (dist.is_available() and dist.is_initialized()):
            return
        buf = self.flat if part == "all" else (self.flat[self.tail_start:] if part == "tail" else self.flat[:self.tail_start])
        if buf.numel() == 0:
            return
        if buf.is_cuda and dist.get_backend(group) == "gloo":
            # gloo has no device collectives here: stage through the host (tests that share ONE GPU between
            # ranks use this; the production backend is "nccl" = RCCL, which reduces the device buffer in place)
            host = buf.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            buf.copy_(host)
        else:
            # eager calls keep their Work handle (async_op + wait() is stream-ordered exactly like the blocking call):
            # TrainStep.capture() polls the LAST eager collective for completion before it starts capturing.  Captured
            # calls stay the plain blocking form.
            if buf.is_cuda and not torch.cuda.is_current_stream_capturing():
                work = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group, async_op=True)
                if work is not None:
                    work.wait()
                    self.last_work = work
            else:
                dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        if average:
            buf.div_(dist.get_world_size(group))


def broadcast_parameters(module: torch.nn.Module, src: int = 0, group=None) -> None:
    """Make every replica start from rank ``src``'s parameters (and buffers)."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    for t in list(module.parameters()) + list(module.buffers()):
        if t.is_cuda and dist.get_backend(group) == "gloo":       # (tests that share one GPU between ranks: through the host)
            host = t.data.cpu()
            dist.broadcast(host, src=src, group=group)
            t.data.copy_(host)
        else:
            dist.broadcast(t.data, src=src, group=group)


def shard_batch(n_items: int, rank: int, world: int) -> slice:
    """Contiguous shard of a global batch for this rank (remainder to the first ranks)."""
    base, rem = divmod(n_items, world)
    start = rank * base + min(rank, rem)
    return slice(start, start + base + (1 if rank < rem else 0))


class FlatAdam:
    """Adam (+ optional CosineAnnealingLR) as ONE fused update over FlatGradients' flat buffers
    (pit_adam_step): same arithmetic as torch.optim.Adam(lr, betas, eps, weight_decay) followed by
    scheduler.step(), with the step counter on the device (hipGraph-replayable, no host sync)."""

    def __init__(self, flat: FlatGradients, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, cosine_t_max: int = 0, eta_min: float = 0.0, zero_grads: bool = False):
        if flat.flat_params is None:
            raise ValueError("FlatAdam needs FlatGradients(..., flatten_params=True)")
        self.flat = flat
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.cosine_t_max, self.eta_min = cosine_t_max, eta_min
        # zero_grads: the update clears each gradient as it consumes it (= optimizer.zero_grad() fused in);
        # engine.TrainStep then skips its own zeroing launch
        self.zero_grads = bool(zero_grads)
        dev = flat.flat.device
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self.step_count = torch.zeros((), device=dev, dtype=torch.int64)
        self.scalars = torch.zeros(4, device=dev, dtype=torch.float32)

    def step(self) -> None:
        from . import _lib, ops
        f = self.flat
        f.attach()
        ops.parameters_changed()            # raw-pointer update: cached host-evaluated head scales are void
        rc = _lib.lib().pit_adam_step(f.flat_params.data_ptr(), f.flat.data_ptr(), self.exp_avg.data_ptr(),
                                      self.exp_avg_sq.data_ptr(), f.flat.numel(), self.step_count.data_ptr(),
                                      self.lr, self.eta_min, self.cosine_t_max, self.betas[0], self.betas[1],
                                      self.eps, self.weight_decay, 1 if self.zero_grads else 0,
                                      self.scalars.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_adam_step")

    # -- state: what an interrupted run needs to go on with the same bits (engine.TrainStep.state_dict saves it with the model)
    def _config(self) -> dict:
        """The settings the saved tensors were produced under, as plain Python numbers."""
        return {"class": type(self).__name__, "n": int(self.flat.flat.numel()), "lr": float(self.lr),
                "beta1": float(self.betas[0]), "beta2": float(self.betas[1]), "eps": float(self.eps),
                "weight_decay": float(self.weight_decay), "cosine_t_max": int(self.cosine_t_max), "eta_min": float(self.eta_min)}

    def _state_tensors(self) -> dict:
        """Every device tensor the step reads and carries from call to call.  Not among them: ``scalars`` (slots 0..2 are
        rewritten by the next step, slot 3 is the arrival ticket and must stay 0) and the guarded step's ``partials`` (scratch)."""
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step_count": self.step_count}

    def state_dict(self) -> dict:
        """CPU copies of the moments and the step counter (subclasses: of every tensor their step carries along), and
        ``config``: the settings as plain numbers.  The parameters are the model's (``model.state_dict()``).  The dict passes
        ``torch.save`` and ``torch.load(weights_only=True)``.  This synchronises."""
        state = {name: t.detach().to("cpu", copy=True) for name, t in self._state_tensors().items()}
        state["config"] = self._config()
        return state

    def load_state_dict(self, state: dict, strict: bool = True) -> None:
        """Copy a ``state_dict()`` back IN PLACE (``copy_``: graphs captured on these tensors stay valid).  ``strict``: every
        ``config`` entry must equal this optimizer's (ValueError naming the first that differs); ``strict=False`` takes the
        tensors alone.  A state of another size is always refused."""
        from . import ops
        own = self._state_tensors()
        missing = [name for name in own if name not in state]
        if missing:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state lacks {', '.join(missing)}")
        config, mine = state.get("config") or {}, self._config()
        if "n" in config and int(config["n"]) != mine["n"]:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state was saved for n = {config['n']} elements, "
                             f"this optimizer has n = {mine['n']}")
        for name, t in own.items():
            if not torch.is_tensor(state[name]) or tuple(state[name].shape) != tuple(t.shape):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {name} has shape "
                                 f"{tuple(getattr(state[name], 'shape', ()))}, this optimizer's {tuple(t.shape)}")
        if strict:
            for name, value in mine.items():
                if name not in config or config[name] != value:
                    raise ValueError(f"{type(self).__name__}.load_state_dict: the state was saved with {name} = "
                                     f"{config.get(name)!r}, this optimizer has {name} = {value!r} (strict=False takes the "
                                     "tensors alone)")
        for name, t in own.items():
            t.copy_(state[name])
        ops.parameters_changed()


# ---- the guarded step: clip, skip, AdamW and warm-up inside the captured step ----------------------------------------------------
def guard_run(n: int) -> int:
    """Elements per partial of the guarded step's gradient norm (include/pit_hip.h, pit_adam_step_guarded)."""
    from . import _lib
    n = int(n)
    if n <= 0:
        raise ValueError(f"n must be positive, got {n}")
    unit = 1024 * _lib.GUARD_MAX_PARTS
    return 1024 * ((n + unit - 1) // unit)


def guard_parts(n: int) -> int:
    """pit_adam_guard_parts on the host: the number of fp64 partials for ``n`` gradients; partial ``b`` covers the elements
    ``[b * guard_run(n), min(n, (b + 1) * guard_run(n)))``."""
    run = guard_run(n)
    return (int(n) + run - 1) // run


def guarded_lr(k: int, lr: float, eta_min: float = 0.0, cosine_t_max: int = 0, warmup_steps: int = 0,
               warmup_start: float = 0.0) -> float:
    """The learning rate of call ``k`` (1-based, skipped calls included) of the guarded step, in fp64: a linear warm-up
    from ``lr * warmup_start`` over the first ``warmup_steps`` calls, then CosineAnnealingLR's closed form counted from
    the end of the warm-up (constant ``lr`` when ``cosine_t_max == 0``)."""
    import math
    k = int(k)
    if k < 1:
        raise ValueError(f"calls are counted from 1, got {k}")
    if k <= warmup_steps:
        return lr * (warmup_start + (1.0 - warmup_start) * (k - 1) / warmup_steps)
    if cosine_t_max > 0:
        return eta_min + 0.5 * (lr - eta_min) * (1.0 + math.cos(math.pi * (k - 1 - warmup_steps) / cosine_t_max))
    return lr


class GuardHealth(NamedTuple):
    """GuardedAdam.health(): the PIT_GUARD_* slots of include/pit_hip.h since the last reset, and the mean of the finite
    losses (NaN when there was none)."""
    calls: int
    applied: int
    skipped: int
    clipped: int
    norm: float
    max_norm: float
    coef: float
    loss_sum: float
    finite_loss: int
    nonfinite_loss: int
    mean_loss: float


class GuardedAdam(FlatAdam):
    """FlatAdam with the look at the gradient that a captured step has lost (pit_adam_step_guarded, two launches, no host
    round trip): the global L2 norm of the flat gradient in fp64, ``torch.nn.utils.clip_grad_norm_``'s coefficient for
    ``max_grad_norm`` (None or 0: no clipping), and NO update at all when the norm is not finite - parameters, moments and
    ``step_count`` keep their bits, the gradients are still cleared with ``zero_grads``, and the skip is counted.
    ``decoupled=True`` is torch.optim.AdamW's decay; ``warmup_steps`` / ``warmup_start`` put a linear warm-up in front of
    the cosine schedule (``guarded_lr``).  The schedule counts every call (``calls``), the bias corrections the applied
    updates (``step_count``).

    In a data-parallel step the guard runs on the all-reduced buffer, so every rank sees the same bits and takes the same
    decision: a NaN on one rank skips the step on all.  ``FlatGradients.all_reduce`` SUMS over the ranks (the loss sums
    over the batch), so ``max_grad_norm`` bounds the norm of the SUMMED gradient - that of the global batch - not of a
    rank's mean.

    ``health()`` is the only call that synchronises."""

    def __init__(self, flat: FlatGradients, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, cosine_t_max: int = 0, eta_min: float = 0.0, zero_grads: bool = False,
                 max_grad_norm: Optional[float] = None, decoupled: bool = False, warmup_steps: int = 0,
                 warmup_start: float = 0.0):
        from . import _lib
        max_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        if not max_norm >= 0.0:
            raise ValueError(f"max_grad_norm must be None or a number >= 0, got {max_grad_norm!r}")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError(f"warmup_steps must be an integer >= 0, got {warmup_steps!r}")
        if not 0.0 <= float(warmup_start) <= 1.0:
            raise ValueError(f"warmup_start must lie in [0, 1], got {warmup_start!r}")
        super().__init__(flat, lr, betas, eps, weight_decay, cosine_t_max, eta_min, zero_grads)
        if flat.flat.dtype != torch.float32:
            raise ValueError("GuardedAdam works on fp32 flat buffers")
        self.max_grad_norm, self.decoupled = max_norm, bool(decoupled)
        self.warmup_steps, self.warmup_start = int(warmup_steps), float(warmup_start)
        dev = flat.flat.device
        # everything the two launches touch exists before any capture
        self.partials = torch.zeros(_lib.GUARD_MAX_PARTS, device=dev, dtype=torch.float64)
        self.state = torch.zeros(_lib.GUARD_STATE_DOUBLES, device=dev, dtype=torch.float64)
        self.calls = torch.zeros((), device=dev, dtype=torch.int64)
        self._loss = None

    def watch_loss(self, loss: Optional[torch.Tensor]) -> None:
        """The device scalar whose value the next ``step()`` adds to the loss statistics (engine.TrainStep hands over the
        step's loss just before ``step()``; None: no loss is recorded)."""
        if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1 or loss.device != self.state.device):
            raise ValueError("watch_loss takes one fp32 scalar on the optimizer's device")
        self._loss = loss

    def step(self) -> None:
        from . import _lib, ops
        f = self.flat
        f.attach()
        ops.parameters_changed()            # raw-pointer update: cached host-evaluated head scales are void
        rc = _lib.lib().pit_adam_step_guarded(
            f.flat_params.data_ptr(), f.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), f.flat.numel(),
            self.step_count.data_ptr(), self.calls.data_ptr(), self.lr, self.eta_min, self.cosine_t_max, self.warmup_steps,
            self.warmup_start, self.betas[0], self.betas[1], self.eps, self.weight_decay, 1 if self.decoupled else 0,
            self.max_grad_norm, 1 if self.zero_grads else 0, _lib.ptr(self._loss), self.partials.data_ptr(),
            self.state.data_ptr(), self.scalars.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pit_adam_step_guarded")

    def health(self, reset: bool = False) -> GuardHealth:
        """The statistics since the last reset, read from the device (this synchronises).  ``reset=True`` zeroes them
        afterwards - the epoch's line; the schedule's position and the bias corrections are not touched."""
        s = self.state.cpu().tolist()
        if reset:
            self.state.zero_()
        n_loss = int(s[8])
        return GuardHealth(int(s[0]), int(s[1]), int(s[2]), int(s[3]), s[4], s[5], s[6], s[7], n_loss, int(s[9]),
                           s[7] / n_loss if n_loss else float("nan"))

    def _config(self) -> dict:
        config = super()._config()
        config.update(max_grad_norm=float(self.max_grad_norm), decoupled=bool(self.decoupled), warmup_steps=int(self.warmup_steps),
                      warmup_start=float(self.warmup_start))
        return config

    def _state_tensors(self) -> dict:
        tensors = super()._state_tensors()
        tensors.update(calls=self.calls, state=self.state)            # the schedule's position and the health slots
        return tensors


# ---- averaged weights: an EMA or equal average of the parameters kept by the guarded step's own two launches ------------------------
_AVERAGE_MODES = {"ema": 0, "equal": 1}


def average_weight(m: int, mode: str = "ema", decay: float = 0.999, ramp: bool = False) -> float:
    """The weight ``w`` of averaged update ``m`` (1-based: the m-th applied update after ``average_start``) in
    ``average += w * (p - average)``, in fp64 as pit_adam_step_averaged forms it (include/pit_hip.h); the kernel's ``w`` is
    ``numpy.float32`` of this.  "ema": ``1 - decay``, with ``ramp`` ``1 - min(decay, (1 + m) / (10 + m))`` (a short average at
    the start of the run); "equal": ``1 / m``.  The counterpart of ``guarded_lr``."""
    m = int(m)
    if m < 1:
        raise ValueError(f"averaged updates are counted from 1, got {m}")
    if mode not in _AVERAGE_MODES:
        raise ValueError(f"mode must be 'ema' or 'equal', got {mode!r}")
    if mode == "equal":
        return 1.0 / float(m)
    d = min(float(decay), (1.0 + float(m)) / (10.0 + float(m))) if ramp else float(decay)
    return 1.0 - d


class AveragedAdam(GuardedAdam):
    """GuardedAdam that also keeps an average of the parameters - what a user evaluates and ships - in the SAME two launches
    (pit_adam_step_averaged): after every applied update, ``average += w * (p - average)`` with ``average_weight``'s ``w``
    (``average="ema"``: exponential with ``average_decay``, ``average_ramp`` for the short average at the start; ``"equal"``:
    the plain mean of the weights after each update, SWA).  Until ``average_start`` updates have been applied the average is a
    copy of the weights.  A skipped call leaves ``average`` and ``n_averaged`` alone, and the average never feeds back into
    the update: parameters, moments, counters and health have GuardedAdam's bits.

    Evaluating it costs one launch each way and no capture: ``with opt.averaged():`` exchanges ``flat_params`` and ``average``
    in place (pit_exchange_words), so every graph that reads the parameters where they live - an engine.EvalStep captured on
    the same model under the 'device' head-scale route - evaluates the average; under the 'host' route such a graph holds the
    scales of the lmda values of its capture and its ``reset()`` refuses, as after any other change of the parameters.  While
    swapped, ``step()``, ``state_dict()`` and ``load_state_dict()`` raise: training would update the average, a checkpoint
    would hold the two buffers crossed."""

    def __init__(self, flat: FlatGradients, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, cosine_t_max: int = 0, eta_min: float = 0.0, zero_grads: bool = False,
                 max_grad_norm: Optional[float] = None, decoupled: bool = False, warmup_steps: int = 0,
                 warmup_start: float = 0.0, average: str = "ema", average_decay: float = 0.999, average_ramp: bool = False,
                 average_start: int = 0):
        if average not in _AVERAGE_MODES:
            raise ValueError(f"average must be 'ema' or 'equal', got {average!r}")
        if average == "ema" and not 0.0 <= float(average_decay) < 1.0:
            raise ValueError(f"average_decay must lie in [0, 1), got {average_decay!r}")
        if int(average_start) != average_start or average_start < 0:
            raise ValueError(f"average_start must be an integer >= 0, got {average_start!r}")
        super().__init__(flat, lr, betas, eps, weight_decay, cosine_t_max, eta_min, zero_grads, max_grad_norm, decoupled,
                         warmup_steps, warmup_start)
        self.average_mode, self.average_decay = average, float(average_decay)
        self.average_ramp, self.average_start = bool(average_ramp), int(average_start)
        # both exist before any capture; the average starts as the weights
        self.average = flat.flat_params.clone()
        self.n_averaged = torch.zeros((), device=flat.flat.device, dtype=torch.int64)
        self.swapped = False

    def _refuse_swapped(self, what: str) -> None:
        if self.swapped:
            raise RuntimeError(f"AveragedAdam.{what} while the average is swapped in (flat_params holds the average, `average` "
                               "the live weights): swap back first (swap_average(), or leave the `with opt.averaged():` block)")

    def step(self) -> None:
        from . import _lib, ops
        self._refuse_swapped("step()")
        f = self.flat
        f.attach()
        ops.parameters_changed()            # raw-pointer update: cached host-evaluated head scales are void
        rc = _lib.lib().pit_adam_step_averaged(
            f.flat_params.data_ptr(), f.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), f.flat.numel(),
            self.step_count.data_ptr(), self.calls.data_ptr(), self.lr, self.eta_min, self.cosine_t_max, self.warmup_steps,
            self.warmup_start, self.betas[0], self.betas[1], self.eps, self.weight_decay, 1 if self.decoupled else 0,
            self.max_grad_norm, 1 if self.zero_grads else 0, _lib.ptr(self._loss), self.partials.data_ptr(),
            self.state.data_ptr(), self.scalars.data_ptr(), self.average.data_ptr(), self.n_averaged.data_ptr(),
            _AVERAGE_MODES[self.average_mode], self.average_decay, 1 if self.average_ramp else 0, self.average_start,
            _lib.stream_ptr())
        _lib.check(rc, "pit_adam_step_averaged")

    def swap_average(self) -> None:
        """Exchange ``flat_params`` and ``average`` in place: one launch (pit_exchange_words), no allocation, addresses do not
        move.  Toggles ``swapped``."""
        from . import _lib, ops
        f = self.flat
        rc = _lib.lib().pit_exchange_words(f.flat_params.data_ptr(), self.average.data_ptr(), f.flat_params.numel(),
                                           _lib.stream_ptr())
        _lib.check(rc, "pit_exchange_words")
        ops.parameters_changed()
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def averaged(self):
        """``with opt.averaged():`` - the model computes with the averaged weights inside the block and with its own after it
        (also when the block raises)."""
        self._refuse_swapped("averaged()")
        self.swap_average()
        try:
            yield self
        finally:
            self.swap_average()

    def averaged_model_state(self, model: torch.nn.Module) -> dict:
        """``model.state_dict()`` with every parameter this optimizer updates replaced by (a copy of) its slice of the average;
        parameters are matched by identity through ``flat.params``, buffers, frozen parameters and key names are untouched:
        ``{'model_state': opt.averaged_model_state(model)}`` loads in the reference scripts and through
        utils.load_reference_checkpoint."""
        f = self.flat
        source = f.flat_params if self.swapped else self.average
        where = {id(p): (off, p.numel()) for p, off in zip(f.params, f.offsets)}
        state = model.state_dict()
        for name, p in model.named_parameters():
            if id(p) in where and name in state:
                off, n = where[id(p)]
                state[name] = source[off:off + n].view_as(p).clone()
        return state

    def _config(self) -> dict:
        config = super()._config()
        config.update(average=self.average_mode, average_decay=float(self.average_decay), average_ramp=bool(self.average_ramp),
                      average_start=int(self.average_start))
        return config

    def _state_tensors(self) -> dict:
        tensors = super()._state_tensors()
        tensors.update(average=self.average, n_averaged=self.n_averaged)
        return tensors

    def state_dict(self) -> dict:
        self._refuse_swapped("state_dict()")
        return super().state_dict()

    def load_state_dict(self, state: dict, strict: bool = True) -> None:
        self._refuse_swapped("load_state_dict()")
        super().load_state_dict(state, strict)
