"""Sync-free training step: forward -> RelLp loss -> backward -> (grad all-reduce) -> (Adam),
captured once into a hipGraph and replayed.

The reference loop calls ``loss.item()`` every step and creates tensors inside forward
(train_darcy.py:124-134, pit.py:50), both capture-hostile; here the loss stays on the
device, every launch goes to the capture stream through the C ABI, and the gradients live
in one flat buffer (ddp.FlatGradients) so a data-parallel step is ONE all-reduce.
"""
from __future__ import annotations

import inspect
from typing import NamedTuple, Optional, Sequence

import torch

from . import ops
from .ddp import FlatGradients


def early_gradient_parameters(model: torch.nn.Module):
    """(parameters, module) for a two-bucket data-parallel step: the weights whose gradients are COMPLETE once the
    backward pass has gone through processor block ``mid = n_blocks // 2`` (pit.py:116-121 in reverse: de, then
    mlp[n-1] ... mlp[mid]; an MLP's weight-gradient reductions ride with the attention backward that follows it,
    ops.MLP_PARAMS_RIDER) and the module whose OUTPUT gradient marks that point (mlp[mid-1]).  The lmda gradients
    are finished by one launch at the end of the pass and stay in the late bucket."""
    mlps, de = getattr(model, "mlp", None), getattr(model, "de", None)
    if mlps is None or de is None or len(mlps) < 2:
        return [], None
    mid = len(mlps) // 2
    params = [p for m in list(mlps[mid:]) + [de] for p in m.parameters() if p.requires_grad]
    return params, mlps[mid - 1]


class _StaticBatch:
    """What the captured steps of this module share: the static length tensors of a ragged batch, the copy of a new batch into
    the static buffers, and the capture procedure.  Expects ``model``, ``mesh_in``, ``func_in``, ``mesh_out``, ``target``,
    ``affine``, ``len_in``, ``len_out``, ``_len_loss`` and ``_len_kw`` on the object."""

    _feed = None         # a DeviceFeed attached to the step: its launch is the first of ``_step``, and ``set_batch`` is refused

    def _refuse_set_batch_with_feed(self) -> None:
        if self._feed is not None:
            raise RuntimeError("set_batch on a step with a DeviceFeed attached: the feed's launch fills the static buffers at the "
                               "head of every step - two sources for the same buffers")

    def _init_lengths(self, len_in, len_out) -> None:
        """The checks of a ragged step (before any launch) and its static length tensors."""
        if self.affine is not None:
            raise ValueError("pred_affine with lengths: a per-pixel affine has no meaning on ragged clouds")
        if isinstance(self, (RolloutStep, RolloutEvalStep)):
            raise ValueError("RolloutStep with lengths: the rollout runs on one fixed mesh")
        params = inspect.signature(self.model.forward).parameters
        any_kw = any(q.kind is inspect.Parameter.VAR_KEYWORD for q in params.values())
        batch = self.func_in.shape[0]
        for name, given in (("len_in", len_in), ("len_out", len_out)):
            if given is None:
                continue
            if not any_kw and name not in params:
                raise ValueError(f"{type(self.model).__name__}.forward does not accept the keyword {name}")
            width = (self.mesh_in if name == "len_in" else self.mesh_out).shape[-2]
            self._check_length_list(name, given, width)
            t = ops.as_lengths(given, self.func_in.device, batch)      # (an int32 device tensor is used as it is)
            setattr(self, name, t)
            self._len_kw[name] = t
        if self.len_out is not None:
            self._len_loss = self.len_out
        elif self.mesh_out is self.mesh_in or (self.mesh_out.data_ptr() == self.mesh_in.data_ptr()
                                                and self.mesh_out.shape == self.mesh_in.shape):
            self._len_loss = self.len_in

    @staticmethod
    def _check_length_list(name: str, lengths, width: int) -> None:
        # a Python sequence is checked on the host; a tensor is taken as it is (a check would synchronise; the kernels clamp)
        if not torch.is_tensor(lengths):
            for n in lengths:
                if not 1 <= int(n) <= width:
                    raise ValueError(f"{name}: length {int(n)} outside [1, {width}]")

    def _check_mesh_update(self, mesh_in, mesh_out) -> None:
        if (mesh_in is not None or mesh_out is not None) and not getattr(self.model.down, "_batched", True):
            raise ValueError("this model's meshes are batch-free (fixed): their selection plans were built once and "
                             "are part of the captured step; only per-sample meshes can change between replays")

    def _set_lengths(self, len_in, len_out) -> None:
        for name, given in (("len_in", len_in), ("len_out", len_out)):
            if given is None:
                continue
            static = getattr(self, name)
            if static is None:
                raise ValueError(f"set_batch({name}=...): this step was built without {name}")
            self._check_length_list(name, given, (self.mesh_in if name == "len_in" else self.mesh_out).shape[-2])
            static.copy_(ops.as_lengths(given, static.device, static.numel()))

    def _capture_graph(self, warmup: int, collective: bool):
        """Warm up (allocator, mesh-plan caches, the per-stream accumulators of ops) and capture ``self._step`` ON THE SAME
        side stream: a workspace first requested during capture would be allocated - and zero-filled by a
        captured memset on every replay - inside the graph.  Returns (graph, stream)."""
        import position_induced_transformer_amd as _pkg
        if not _pkg.GRAPH_PACKET_CAPTURE_OFF and getattr(getattr(self.model, "down", None), "_batched", False):
            raise RuntimeError("this step builds per-sample selection plans inside the graph, which faults on replay with "
                               "ROCm 7.2's hipGraph packet capture; DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 was not in effect "
                               "when the HIP runtime started (import position_induced_transformer_amd, or export the "
                               "variable, before the first .cuda() call) - run the step eagerly or restart")
        side = torch.cuda.Stream()
        # (a feed's cursor is put back where it was before the warm-up passes: a device copy on either side of them)
        cursor = self._feed.state.clone() if self._feed is not None else None
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step()
            if cursor is not None:
                self._feed.state.copy_(cursor)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # A data-parallel step is captured in THREAD-LOCAL error mode, after the process group's watchdog has let go of
        # the warm-up collectives.  That thread polls the events of every collective issued so far with hipEventQuery
        # every 100 ms until it has seen them complete.  Under the default global mode HIP refuses the query while ANY
        # stream captures ("operation not permitted when stream is capturing") and, in every mode, for an event whose
        # stream has since JOINED a capture - as RCCL's internal stream does when the step's all-reduce is captured
        # (tools/micro/capture_query_probe.py).  The watchdog rethrows and the process aborts: one capture in eight on
        # MI355X, when a poll fell inside the capture window.  All work is complete after the synchronize above; a few
        # poll periods later the watchdog's list is empty.  Launches from autograd's worker thread are still captured:
        # the mode only decides whose unsafe calls are refused, not what the stream records.
        mode = "global"
        if collective:
            mode = "thread_local"
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_backend() != "gloo":
                # wait until the watchdog can have nothing left to poll: the last warm-up collective reports completion
                # (bounded), then three of the watchdog's 100 ms periods for it to retire the entry
                import time
                work, t0 = getattr(self.flat, "last_work", None), time.monotonic()
                while work is not None and not work.is_completed() and time.monotonic() - t0 < 5.0:
                    time.sleep(0.005)
                time.sleep(0.3)
        with torch.cuda.graph(graph, stream=side, capture_error_mode=mode):
            self._step()
        return graph, side


class TrainStep(_StaticBatch):
    def __init__(self, model: torch.nn.Module, batch: Sequence[torch.Tensor], out_dim: int, p: int,
                 pred_affine: Optional[Sequence[torch.Tensor]] = None, all_reduce: bool = False,
                 optimizer: Optional[torch.optim.Optimizer] = None, flat: Optional[FlatGradients] = None,
                 all_reduce_buckets: int = 1, len_in=None, len_out=None):
        """``all_reduce_buckets=2``: the gradient exchange is split - the bucket of weights whose gradients are
        complete half-way through the backward pass (early_gradient_parameters) is all-reduced on a second stream
        while the rest of the backward runs, the remainder after the pass; needs a ``flat`` built with that
        bucket as its ``tail`` (done here when ``flat`` is None).

        ``len_in`` / ``len_out`` (lists or tensors, one entry per sample): a ragged batch of padded clouds
        (tasks.pit_elasticity, tasks.pit_cloud_latent).  Each becomes a static int32 device tensor (``self.len_in`` /
        ``self.len_out``) the model is called with and ``set_batch`` overwrites in place, so one captured graph serves every
        mix of sizes up to the padded width.  The loss runs over ``len_out`` - over ``len_in`` when only that is given and
        ``mesh_out`` is ``mesh_in``, the rule of the two task forwards - in ONE launch that also writes its own gradient
        and clears the flat gradient buffer (ops.rel_lp_loss_ragged)."""
        self.model = model
        self.mesh_in, self.func_in, self.mesh_out, self.target = batch
        self.out_dim, self.p = out_dim, p
        self.affine = pred_affine
        self.len_in = self.len_out = self._len_loss = None
        self._len_kw = {}
        if len_in is not None or len_out is not None:
            self._init_lengths(len_in, len_out)
        self.all_reduce = all_reduce
        self.optimizer = optimizer
        self.buckets = 1
        self._early_hook = None
        if all_reduce_buckets == 2:
            tail, marker = early_gradient_parameters(model)
            if marker is not None:
                if flat is None:
                    flat = FlatGradients(model.parameters(), tail=tail)
                if flat.tail_start < flat.flat.numel() and \
                        {id(q) for q in flat.params[len(flat.params) - len(tail):]} == {id(q) for q in tail}:
                    self.buckets = 2
                    self._tail_params = list(tail)
                    self._early_block = len(model.mlp) // 2      # after this block's backward its bucket is complete
                    self._side = None                            # second stream of the early exchange: created at its first use

                    def mark(module, inputs, output):      # (a plain function: it carries the marker attribute)
                        return self._mark_early_point(module, inputs, output)
                    mark._pit_internal = True              # pit._fused_processor: not a user hook, fusing stays allowed
                    self._early_hook = marker.register_forward_hook(mark)
        elif all_reduce_buckets not in (1, 2):
            raise ValueError("all_reduce_buckets must be 1 or 2")
        self.flat = flat if flat is not None else FlatGradients(model.parameters())
        self._early_pending = False
        self._early_ok = False
        self._early_decision = None          # two buckets or one exchange: decided ONCE, by all ranks together (_agree_early)
        self.loss = torch.zeros((), device=self.func_in.device)
        self.out = None
        self._seed = torch.ones((), device=self.func_in.device)      # d loss / d loss, allocated once
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._agree_early()                  # (a collective when the process group has more than one rank: every rank builds its step)

    # two-bucket exchange: when the gradient of the marker module's output arrives, everything after it in the forward
    # has been back-propagated (launches enqueued) - fork the second stream there and reduce the early bucket on it
    def _tail_in_place(self) -> bool:
        """The early bucket may only be reduced before the pass ends if every one of its gradients is WRITTEN IN PLACE by
        the kernels (ops._grad_slot): a parameter with a hook, a dropped / replaced .grad, or FUSED_GRAD_ACCUMULATION off
        gets its gradient from autograd's AccumulateGrad AFTER the node returns - for the fused processor that is after the
        early all-reduce was issued, and the ranks would silently diverge."""
        return all(ops._grad_slot(p) is not None for p in self._tail_params)

    def _agree_early(self) -> None:
        """Two-bucket exchange or one all-reduce after the pass: the SHAPE of the collective sequence.  Decided ONCE, when the
        step object is built, by all ranks together: EVERY rank of a data-parallel step enters the MIN all-reduce below,
        whatever its own bucket count - a rank that ended with one bucket (no marker module, a caller-supplied ``flat`` without
        the tail layout, a hook on a tail parameter, a dropped .grad, another FUSED_GRAD_ACCUMULATION setting) contributes 0
        and every rank then issues ONE all-reduce per step.  (Round 5 ran the agreement lazily in the first ``_step`` and only
        on ranks with two buckets: a rank with one skipped the collective its peers blocked in, and ``capture(warmup=0)`` put
        a collective and a host sync inside the stream capture - ADVICE r5.)"""
        local = bool(self.buckets == 2 and self._tail_in_place())
        agreed = local
        if self.all_reduce:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                flag = torch.tensor([1 if local else 0], device=self.func_in.device if dist.get_backend() != "gloo" else "cpu",
                                    dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                agreed = bool(int(flag.item()))
        else:
            agreed = False                   # (no exchange at all: nothing to split)
        self._early_decision = agreed

    def _decide_early(self) -> bool:
        """The agreed shape (``_agree_early``); raises if the local condition it rested on stopped holding - a captured graph has
        the shape it was captured with baked in, and the other ranks keep theirs."""
        if self._early_decision is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TrainStep: the collective sequence was never agreed on (the step object was not built by "
                                   "__init__?) - refusing to run a collective and a host sync inside a stream capture")
            self._agree_early()
        if self._early_decision and not (self.buckets == 2 and self.all_reduce and self._tail_in_place()):
            raise RuntimeError("two-bucket data-parallel step: a gradient of the early bucket is no longer written in place (a hook "
                               "on the parameter, a dropped / replaced .grad, in-place accumulation switched off) - the ranks "
                               "agreed on the two-bucket exchange when the step was built; rebuild the TrainStep")
        return self._early_decision

    def _mark_early_point(self, _module, _inputs, output):
        if self._early_ok and torch.is_tensor(output) and output.requires_grad:
            output.register_hook(self._reduce_early_bucket)

    def _reduce_early_bucket(self, _grad):
        if not self._early_pending:
            self._early_pending = True
            cur = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.func_in.device)
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                self.flat.all_reduce(part="tail")
        return None

    def _exchange_gradients(self) -> None:
        if self.buckets == 2 and self._early_pending:
            self.flat.all_reduce(part="head")
            torch.cuda.current_stream().wait_stream(self._side)
            self._early_pending = False
        else:
            self.flat.all_reduce()

    def _on_processor_block(self, i: int) -> None:
        # the fused processor (ops._Processor) is one autograd node: it reports each block's backward launch instead
        if i == self._early_block:
            self._reduce_early_bucket(None)

    def _step(self) -> None:
        if self._feed is not None:
            self._feed.launch()                  # the step's FIRST launch: this step's samples into the static buffers
        self._early_pending = False
        early = self._decide_early()             # (False: ONE all-reduce after the pass)
        self._early_ok = early
        sc, sh = self.affine if self.affine is not None else (None, None)
        # the flat gradient accumulators are cleared on the way by the step's first fused launch (ops.encoder_apply) or by
        # the loss launch (unless FlatAdam(zero_grads=True) already did): no memset launch
        clear = None if getattr(self.optimizer, "zero_grads", False) else self.flat.flat
        # the loss the step applies to the prediction: a fused decoder accumulates its partial sums in the forward launch and
        # forms d(pred) in the backward launch - no loss launch (ops.LossSpec; any other model, and the reproducible mode, run the
        # loss kernel below)
        # (a ragged step builds none: its loss runs over the lengths)
        spec = ops.LossSpec(self.target, sc, sh, self.out_dim, self.p) if self.p in (1, 2) and ops.EDGE_FUSION and not ops.reproducible_wanted() and not self._len_kw else None
        # per-thread state, read by the autograd nodes in their forward (ops._STEP)
        with ops.step_state(processor_hook=(self._on_processor_block, self._early_block) if early else None, loss=spec, clear=clear):
            self._step_body(sc, sh)

    def _step_body(self, sc, sh) -> None:
        out = self.model(self.mesh_in, self.func_in, self.mesh_out, **self._len_kw)
        clear = ops.take_pending_clear()         # None when a launch of the forward already zeroed the buffer
        # the loss launch also writes its own gradient for the seed of ones below: no loss-backward launch
        if self._len_loss is not None:
            loss = ops.rel_lp_loss_ragged(self.target, out, self._len_loss, self.out_dim, self.p, unit_seed=self._seed, clear=clear)
        else:
            loss = ops.rel_lp_loss(self.target, out, self.out_dim, self.p, sc, sh, unit_seed=self._seed, clear=clear)
        torch.autograd.backward(loss, grad_tensors=self._seed)        # no ones_like fill per step
        self.loss = loss.detach()            # same storage every replay (graph-private pool): no copy
        self.out = out.detach()              # (the prediction of the last step / replay: parity checks read it)
        if self.all_reduce:
            self._exchange_gradients()
        self._optimizer_step()

    def _optimizer_step(self) -> None:
        if self.optimizer is not None:
            # ddp.GuardedAdam looks at the all-reduced gradient (every rank decides alike) and keeps the loss statistics
            watch = getattr(self.optimizer, "watch_loss", None)
            if watch is not None:
                watch(self.loss)
            self.optimizer.step()          # torch optimizer (capturable) or ddp.FlatAdam / GuardedAdam (fused HIP step)

    def health(self, reset: bool = False):
        """The optimizer's ``health(reset)`` (ddp.GuardedAdam: norm, clip and skip statistics and the epoch's mean loss, read
        from the device - the one synchronising call of an epoch)."""
        health = getattr(self.optimizer, "health", None)
        if health is None:
            raise RuntimeError("health() needs an optimizer that keeps statistics on the device (ddp.GuardedAdam)")
        return health(reset)

    def run_eager(self) -> None:
        self._step()

    def capture(self, warmup: int = 3) -> None:
        """Warm up and capture the step on one side stream (``_StaticBatch._capture_graph``).  The warm-up passes are real
        steps: they move the optimizer (a feed's cursor is put back).  To resume a saved run, therefore: build, ``capture()``,
        THEN ``load_state_dict()`` - the load overwrites what the warm-up did, in place, and the graph stays valid."""
        graph, side = self._capture_graph(warmup, self.all_reduce)
        ops.assert_frozen_since_capture()     # route 'host': the graph must not update an lmda whose scale it baked in
        self.graph = graph
        self._capture_stream = side

    def replay(self) -> None:
        self.graph.replay()
        if self.optimizer is not None:
            ops.parameters_changed()          # the replay rewrote the parameters behind autograd's back

    def state_dict(self) -> dict:
        """Everything a run needs to go on where it stopped, as CPU copies (this synchronises): ``{"format": 1, "model_state":
        model.state_dict() (the reference's key names, train_darcy.py:150), "optimizer": the optimizer's state_dict()
        (ddp.FlatAdam / GuardedAdam / AveragedAdam: moments, counters, health slots, average; a torch optimizer: its own; None
        without one), "feed": the attached DeviceFeed's (None without one)}``.  Passes ``torch.save`` and, with the fused
        optimizers, ``torch.load(weights_only=True)``.  Valid before or after ``capture()``."""
        model_state = {k: v.detach().to("cpu", copy=True) for k, v in self.model.state_dict().items()}
        return {"format": 1, "model_state": model_state,
                "optimizer": self.optimizer.state_dict() if self.optimizer is not None else None,
                "feed": self._feed.state_dict() if self._feed is not None else None}

    def load_state_dict(self, state: dict, strict: bool = True) -> None:
        """Put a ``state_dict()`` back: the model (in place - its parameters are views of ``flat_params``), the optimizer and the
        feed, then ops.parameters_changed().  Valid before or after ``capture()``; because ``capture()``'s warm-up passes move the
        optimizer, the order of a resume is build, capture, load.  The fused optimizers load in place (captured graphs stay
        valid) and take ``strict`` (ddp.FlatAdam.load_state_dict); a torch optimizer's own ``load_state_dict`` replaces its
        state tensors, so load it BEFORE the capture.  A state with an optimizer or a feed loaded into a step without one (or
        the reverse) is refused."""
        from .ddp import FlatAdam
        if not isinstance(state, dict) or state.get("format") != 1:
            raise ValueError("load_state_dict: not a TrainStep.state_dict() of format 1")
        for name, mine in (("optimizer", self.optimizer), ("feed", self._feed)):
            if (state.get(name) is None) != (mine is None):
                raise ValueError(f"load_state_dict: the state has {'no' if state.get(name) is None else 'an'} {name} state, "
                                 f"this step has {'no' if mine is None else 'an'} {name}")
        self.model.load_state_dict(state["model_state"], strict=strict)
        if self.optimizer is not None:
            if isinstance(self.optimizer, FlatAdam):
                self.optimizer.load_state_dict(state["optimizer"], strict=strict)
            else:
                self.optimizer.load_state_dict(state["optimizer"])
        if self._feed is not None:
            self._feed.load_state_dict(state["feed"])
        ops.parameters_changed()

    def set_batch(self, func_in: torch.Tensor, target: torch.Tensor, mesh_in: Optional[torch.Tensor] = None,
                  mesh_out: Optional[torch.Tensor] = None, len_in=None, len_out=None) -> None:
        """Copy a new batch into the captured static buffers.  Tasks with per-sample meshes
        (train_elasticity.py:46, train_naca.py:62-65) also pass the batch's meshes: the captured step
        rebuilds its selection plans from the static mesh buffers on every replay, so a replay after
        ``set_batch`` computes on the new clouds.  (When mesh_in and func_in are one tensor, as in
        NACA, one copy serves both.)  ``len_in`` / ``len_out``: the new clouds' point counts, copied into the
        step's static length tensors; a list is range-checked here, a tensor is copied unchecked (a check would
        synchronise; the kernels clamp)."""
        self._refuse_set_batch_with_feed()
        self._check_mesh_update(mesh_in, mesh_out)
        self._set_lengths(len_in, len_out)
        self.func_in.copy_(func_in)
        self.target.copy_(target)
        if mesh_in is not None and self.mesh_in.data_ptr() != self.func_in.data_ptr():
            self.mesh_in.copy_(mesh_in)
        if mesh_out is not None and self.mesh_out.data_ptr() != self.mesh_in.data_ptr():
            self.mesh_out.copy_(mesh_out)


class RolloutStep(TrainStep):
    """The autoregressive optimiser step of train_vorticity.py:118-129 as ONE hipGraph: ``steps`` forward
    passes (each prediction appended to the input history), the summed RelLp loss with the script's
    argument order ``myloss(out, y_t)``, one backward through the whole rollout, (all-reduce), (Adam).
    ``batch`` = (mesh, x, y) with x (b, .., memory) and y (b, .., steps)."""

    def __init__(self, model, batch, steps: int, out_dim: int, p: int, recompute: bool = False, **kw):
        mesh, x, y = batch
        kw["all_reduce_buckets"] = 1         # the model is applied `steps` times: its weights' gradients complete at the end
        super().__init__(model, (mesh, x, mesh, y), out_dim, p, **kw)
        self.steps, self.recompute = steps, recompute

    def _step(self) -> None:
        from .tasks import rollout_loss
        if self._feed is not None:
            self._feed.launch()
        clear = None if getattr(self.optimizer, "zero_grads", False) else self.flat.flat
        if clear is not None:
            clear.zero_()
        loss = rollout_loss(self.model, self.mesh_in, self.func_in, self.target, self.steps,
                            lambda out, y_t: ops.rel_lp_loss(out, y_t, self.out_dim, self.p), self.recompute)
        torch.autograd.backward(loss, grad_tensors=self._seed)
        self.loss = loss.detach()
        if self.all_reduce:
            self.flat.all_reduce()
        self._optimizer_step()


# ---- the other half of the epoch: captured evaluation passes ----------------------------------------------------------------------
class EvalResult(NamedTuple):
    """What a pass reports: the SUMS of RelLpNorm / RelMaxNorm over the samples seen (the scripts divide by ntest,
    train_darcy.py:144), the worst sample of each, and the number of samples."""
    rel_lp: float
    rel_max: float
    worst_rel_lp: float
    worst_rel_max: float
    count: int


def merge_eval_state(state: torch.Tensor, group=None) -> torch.Tensor:
    """The evaluation state (ops.eval_metrics: 8 doubles) of every rank of ``group`` combined: the sums [0], [1], the cursor [4]
    and the launch count [5] with SUM, the two worst values [2], [3] with MAX.  Returns a new tensor on ``state``'s device (which
    must be one the group's backend reduces: CPU for gloo); without an initialised process group, a copy."""
    import torch.distributed as dist
    merged = state.detach().clone()
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return merged
    worst = merged[2:4].clone()
    dist.all_reduce(merged, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(worst, op=dist.ReduceOp.MAX, group=group)
    merged[2:4] = worst
    return merged


class EvalStep(_StaticBatch):
    """The evaluation loop of the reference scripts (train_darcy.py:136-144: model.eval(), no_grad, ``myloss(y, out).item()`` per
    test batch) as ONE hipGraph per batch and ONE device->host copy per pass: forward, then one ops.eval_metrics launch that adds
    RelLpNorm and RelMaxNorm of the batch to a state on the device, writes the per-sample errors and (``store_pred``) the
    predictions at the pass's running row cursor.

        step = EvalStep(model, (mesh_in, func_in, mesh_out, target), out_dim, p, capacity=ntest); step.capture()
        step.reset()
        for x, y in loader: step.set_batch(x, y, n_valid=len(x)); step.replay()
        r = step.result()          # r.rel_lp / r.count: the script's test error

    ``pred_is_true``: the model output goes into the metric's ``true`` slot (``myloss(out, y)``, train_vorticity.py:139).
    ``len_in`` / ``len_out``: a ragged batch, as for TrainStep (the metric runs over the same lengths the loss would)."""

    def __init__(self, model: torch.nn.Module, batch: Sequence[torch.Tensor], out_dim: int, p: int,
                 pred_affine: Optional[Sequence[torch.Tensor]] = None, capacity: int = 0, store_pred: bool = False,
                 pred_is_true: bool = False, len_in=None, len_out=None):
        self.model = model
        self.mesh_in, self.func_in, self.mesh_out, self.target = batch
        self.out_dim, self.p = int(out_dim), int(p)
        self.affine = pred_affine
        self.pred_is_true = bool(pred_is_true)
        if self.pred_is_true and pred_affine is not None:
            raise ValueError("pred_affine with pred_is_true: the affine belongs to the metric's `pred` slot, which then holds the target")
        self.capacity = int(capacity)
        if self.capacity < 0:
            raise ValueError("capacity must not be negative")
        if store_pred and self.capacity == 0:
            raise ValueError("store_pred needs a capacity (the rows of the result array)")
        self.len_in = self.len_out = self._len_loss = None
        self._len_kw = {}
        if len_in is not None or len_out is not None:
            self._init_lengths(len_in, len_out)
        dev = self.func_in.device
        self.batch = self.func_in.shape[0]
        self.state = ops.new_eval_state(dev)
        self.n_valid = torch.full((1,), self.batch, device=dev, dtype=torch.int32)
        self._tables(store_pred)
        self.out = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._captured_params = None
        self._captured_host_scales = None

    def _npts(self) -> int:
        return self.target.numel() // (self.batch * self.out_dim)

    def _tables(self, store_pred: bool) -> None:
        dev = self.func_in.device
        self.per_sample = torch.zeros((self.capacity, 2), device=dev) if self.capacity else None
        self.pred = torch.zeros((self.capacity, self._npts(), self.out_dim), device=dev) if store_pred else None

    def _step(self) -> None:
        if self._feed is not None:
            self._feed.launch()                  # (also writes ``n_valid`` for the pass's last, partly filled batch)
        with torch.no_grad():
            out = self.model(self.mesh_in, self.func_in, self.mesh_out, **self._len_kw)
            sc, sh = self.affine if self.affine is not None else (None, None)
            true, pred = (out, self.target) if self.pred_is_true else (self.target, out)
            ops.eval_metrics(true, pred, self.out_dim, self.p, self.state, sc, sh, lengths=self._len_loss, n_valid=self.n_valid,
                             per_sample=self.per_sample, pred_store=self.pred, advance=True, store_true=self.pred_is_true)
            self.out = out               # (the prediction of the last step / replay)

    def run_eager(self) -> None:
        self._step()

    def capture(self, warmup: int = 3) -> None:
        """``TrainStep.capture``'s procedure (``_StaticBatch._capture_graph``).  The warm-up passes move the state; ``reset()``
        starts the pass.  What the graph depends on is recorded for ``reset()``: every parameter's address and - route 'host' -
        the lmda versions whose host-evaluated scales were baked in."""
        ops._STEP.cap_fresh = None        # the bf16 weight casts this graph needs are recorded in THIS graph
        graph, side = self._capture_graph(warmup, False)
        self._captured_host_scales = ([(lmda, version) for lmda, version in ops._HOSTC_CAPTURE["log"]], ops._PARAM_EPOCH[0])
        ops.assert_frozen_since_capture()
        self._captured_params = [(q, q.data_ptr()) for q in self.model.parameters()]
        self.graph = graph
        self._capture_stream = side
        self._graph_out = self.out

    def replay(self) -> None:
        self.graph.replay()
        self.out = self._graph_out        # (an eager run since the capture left its own tensor here)

    def reset(self) -> None:
        """Start a pass: zero the sums, the worst values and the cursor (no synchronisation; rows of ``per_sample`` / ``pred``
        beyond a pass's count keep what earlier passes, the warm-up of ``capture`` among them, wrote; an attached DeviceFeed is sent
        back to position 0).  Once per pass this is also the
        check that the captured graph still evaluates the CURRENT model: it raises when a parameter no longer lives where the
        graph reads it, and when the graph holds host-evaluated head scales (route 'host') of an lmda that changed since."""
        if self.graph is not None:
            for q, addr in self._captured_params:
                if q.data_ptr() != addr:
                    raise RuntimeError("EvalStep: a parameter was moved after the capture (a FlatGradients(flatten_params=True) built "
                                       "later, .to(), a replaced .data): the graph still reads the old storage - capture again")
            log, epoch = self._captured_host_scales
            if log and (epoch != ops._PARAM_EPOCH[0] or any(lmda._version != version for lmda, version in log)):
                raise RuntimeError("EvalStep: this graph was captured with head-scale route 'host' and holds the scales of the lmda "
                                   "values of that moment; the parameters changed since (an optimizer step, a replayed training "
                                   "graph, load_state_dict) - capture again, or capture with the 'device' route")
        self.state.zero_()
        if self._feed is not None:
            self._feed.seek(0)                   # (a device fill: the pass starts at the head of the dataset)

    def set_batch(self, func_in: torch.Tensor, target: torch.Tensor, mesh_in: Optional[torch.Tensor] = None,
                  mesh_out: Optional[torch.Tensor] = None, len_in=None, len_out=None, n_valid: Optional[int] = None) -> None:
        """``TrainStep.set_batch``, and ``n_valid``: how many samples of this batch count (an int in [0, batch], checked here;
        it reaches the device as a fill of a static int32 scalar, no synchronisation; None = the whole batch).  The tensors of a
        partly filled batch may have ``n_valid`` rows only: the other samples keep what they held and are never read by the
        metric."""
        self._refuse_set_batch_with_feed()
        n = self.batch if n_valid is None else int(n_valid)
        if not 0 <= n <= self.batch:
            raise ValueError(f"n_valid {n} outside [0, {self.batch}]")
        self._check_mesh_update(mesh_in, mesh_out)
        if len_in is not None and not torch.is_tensor(len_in) and len(len_in) == n < self.batch:
            len_in = list(len_in) + [1] * (self.batch - n)
        if len_out is not None and not torch.is_tensor(len_out) and len(len_out) == n < self.batch:
            len_out = list(len_out) + [1] * (self.batch - n)
        self._set_lengths(len_in, len_out)

        def put(static, new):
            if new.shape[0] == n < self.batch:
                static[:n].copy_(new)
            else:
                static.copy_(new)
        put(self.func_in, func_in)
        put(self.target, target)
        if mesh_in is not None and self.mesh_in.data_ptr() != self.func_in.data_ptr():
            put(self.mesh_in, mesh_in)
        if mesh_out is not None and self.mesh_out.data_ptr() != self.mesh_in.data_ptr():
            put(self.mesh_out, mesh_out)
        self.n_valid.fill_(n)

    def result(self, all_reduce: bool = False) -> EvalResult:
        """The pass so far: ONE device->host copy of the state (the only synchronisation of a pass).  ``all_reduce``: combined over
        the ranks of the default process group (``merge_eval_state``)."""
        state = self.state
        if all_reduce:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                state = merge_eval_state(state.cpu() if dist.get_backend() == "gloo" else state)
        host = state.cpu().tolist()
        return EvalResult(host[0], host[1], host[2], host[3], int(round(host[4])))


class RolloutEvalStep(EvalStep):
    """The autoregressive evaluation loop of train_vorticity.py:133-141 as ONE hipGraph: ``steps`` forward passes under no_grad,
    each prediction appended to the input history (tasks.rollout_loss), one ops.eval_metrics launch per step with the script's
    argument order ``myloss(out, y_t)``; the last launch moves the cursor.  ``batch`` = (mesh, x, y) with x (b, .., memory) and
    y (b, .., steps).  ``per_sample`` is (capacity, steps, 2), ``pred`` (capacity, steps, npts, out_dim); ``result()`` holds the
    sums over steps and samples (the script divides by ntest * steps) and ``count`` the samples."""

    def __init__(self, model, batch, steps: int, out_dim: int, p: int, capacity: int = 0, store_pred: bool = False):
        mesh, x, y = batch
        self.steps = int(steps)
        if self.steps < 1:
            raise ValueError("steps must be positive")
        super().__init__(model, (mesh, x, mesh, y), out_dim, p, capacity=capacity, store_pred=store_pred, pred_is_true=True)

    def _npts(self) -> int:
        return self.target.numel() // (self.batch * self.out_dim * self.steps)

    def _tables(self, store_pred: bool) -> None:
        dev = self.func_in.device
        self.per_sample = torch.zeros((self.capacity, self.steps, 2), device=dev) if self.capacity else None
        self.pred = torch.zeros((self.capacity, self.steps, self._npts(), self.out_dim), device=dev) if store_pred else None

    def _step(self) -> None:
        if self._feed is not None:
            self._feed.launch()
        with torch.no_grad():
            x, y = self.func_in, self.target
            for t in range(self.steps):
                out = self.model(self.mesh_in, x, self.mesh_in)
                ops.eval_metrics(out, y[..., t:t + 1], self.out_dim, self.p, self.state, n_valid=self.n_valid,
                                 per_sample=self.per_sample[:, t] if self.per_sample is not None else None,
                                 pred_store=self.pred[:, t] if self.pred is not None else None,
                                 advance=(t == self.steps - 1), store_true=True)
                x = torch.cat((x[..., 1:], out), dim=-1)
            self.out = out


# ---- the data feed: the dataset on the device, the batch gathered inside the captured step ------------------------------------------
_M32 = 0xFFFFFFFF
_FEED_ORDERS = {}          # (n, seed, epoch) -> the permutation (a few epochs are kept; expected_indices asks again and again)


def _fmix(h):
    """fmix of include/pit_hip.h on uint32 values held in a uint64 numpy array (or an int)."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def _keyed_permutation(n: int, seed: int, epoch: int):
    """The arithmetic of ``feed_order`` (n >= 1, seed below 2^64, epoch below 2^32): a uint64 numpy array."""
    import numpy as np
    bits = max(2, (n - 1).bit_length())
    bits += bits & 1
    half = bits // 2
    mask = (1 << half) - 1
    lo, hi = seed & _M32, seed >> 32
    keys = [_fmix(lo ^ _fmix((hi + 0x9E3779B9 * (epoch + 1) + j) & _M32)) for j in range(4)]
    x = np.arange(n, dtype=np.uint64)
    todo = np.arange(n)
    while todo.size:                                                   # cycle walking: the entries still outside [0, n)
        v = x[todo]
        left, right = v >> np.uint64(half), v & np.uint64(mask)
        for key in keys:
            left, right = right, left ^ (_fmix((right + np.uint64(key)) & np.uint64(_M32)) & np.uint64(mask))
        v = (left << np.uint64(half)) | right
        x[todo] = v
        todo = todo[v >= n]
    return x


def feed_order(n: int, seed: int, epoch: int) -> torch.Tensor:
    """The keyed permutation of ``range(n)`` that pit_batch_feed applies in epoch ``epoch`` (include/pit_hip.h), restated on the
    host bit for bit: entry g is the sample at position g of the epoch.  A LongTensor on the CPU; needs no GPU.  Four Feistel
    rounds with cycle walking: a bijection for every n, not a Fisher-Yates shuffle in quality (pass ``order`` to DeviceFeed for
    a sampler of your own)."""
    import numpy as np
    n, seed, epoch = int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & _M32
    if n < 1:
        raise ValueError("feed_order: n must be positive")
    hit = _FEED_ORDERS.get((n, seed, epoch))
    if hit is not None:
        return hit.clone()
    out = torch.from_numpy(_keyed_permutation(n, seed, epoch).astype(np.int64))
    if len(_FEED_ORDERS) >= 8:
        _FEED_ORDERS.pop(next(iter(_FEED_ORDERS)))
    _FEED_ORDERS[(n, seed, epoch)] = out
    return out.clone()


def feed_points(length: int, m: int, seed: int, epoch: int, sample: int, group: int = 0) -> torch.Tensor:
    """The points of a cloud that pit_batch_feed_points delivers (include/pit_hip.h), restated on the host bit for bit: of
    sample ``sample``'s cloud of ``length`` real points, in epoch ``epoch``, for point group ``group`` (0: mesh_in / func_in,
    1: mesh_out / target), the ``min(m, length)`` source points in the order they arrive.  It is the head of
    ``feed_order(length, key, epoch)`` with ``key = seed ^ ((sample + 1) * 0x9E3779B97F4A7C15 + group * 0xD1B54A32D192ED03)``
    (mod 2^64): a function of (seed, epoch, sample, group) alone, so a resumed run draws the same subsets.  A LongTensor on
    the CPU; needs no GPU.  (Not kept in ``feed_order``'s cache: every sample has a key of its own.)"""
    length, m, sample, group = int(length), int(m), int(sample), int(group)
    if length < 1 or m < 1:
        raise ValueError("feed_points: length and m must be positive")
    if sample < 0 or group not in (0, 1):
        raise ValueError("feed_points: sample must not be negative and group is 0 or 1")
    key = (int(seed) ^ ((sample + 1) * 0x9E3779B97F4A7C15 + group * 0xD1B54A32D192ED03)) & 0xFFFFFFFFFFFFFFFF
    import numpy as np
    return torch.from_numpy(_keyed_permutation(length, key, int(epoch) & _M32)[:min(m, length)].astype(np.int64))


class DeviceFeed:
    """The data loader of a captured step, on the device: the dataset lives in device memory, and ONE launch at the head of the
    step (ops.batch_feed) picks the step's samples - this rank's shard of a keyed permutation of the current epoch
    (``feed_order``), of the identity (``shuffle=False``) or of the caller's ``order`` - gathers their rows into the step's
    static buffers and moves a cursor that lives on the device.  An epoch, or a whole run, is then

        feed = DeviceFeed(step, {"func_in": x_train, "target": y_train}, seed=0); step.capture()
        for _ in range(epochs * feed.steps_per_epoch): step.replay()

    with no host data traffic and no synchronisation (the loop of train_darcy.py:98,124-126 without loader, ``.cuda()`` and
    ``set_batch``).  ``data`` maps names of the step's static buffers (``FIELDS``) to device tensors with a leading sample axis;
    two names whose static buffers share storage are one field (NACA's mesh_in / func_in: the rule of ``set_batch``) and must
    bring the same tensor.  With
    ``drop_last=False`` (evaluation steps only: they have ``n_valid``) the last step of an epoch is partly filled: the launch
    writes the step's ``n_valid`` and fills the remaining slots with samples from the head of the order, so the forward never
    reads garbage.  Data-parallel: global position ``(i * world_size + rank) * batch + s`` for slot s of step i, so the ranks of
    one step hold disjoint runs of the same order.  Attach the feed BEFORE ``capture()``.

    ``subsample=True``: every step sees a random subset of each cloud's points (ops.batch_feed_points, still one launch).
    ``mesh_in``, ``func_in``, ``mesh_out`` and ``target`` are then point fields: data ``(N, n, ...)`` against the step's static
    ``(batch, m, ...)`` with ``m <= n``; mesh_in / func_in form group 0, mesh_out / target group 1 (one group, which ``target``
    follows, when the step's mesh_out shares storage with its mesh_in), and every field of a group receives the same subset -
    ``feed_points(length, m, seed, epoch, sample, group)``, new in every epoch, in permutation order (the layers do not depend
    on the order of the points except in the order of their sums; ``pit_cloud_fps(start=0)`` then starts from a random point
    of the cloud).  ``len_in`` / ``len_out`` in ``data`` are the SOURCE lengths: points beyond them are never read.  A step built
    with lengths receives ``min(m, length)`` per slot (``m`` when the data has no lengths) and zero rows beyond; a step built
    without needs ``m`` points in the shortest cloud, checked once here.  A sample that a caller's ``order`` repeats within an
    epoch repeats its subset.  ``points_in`` / ``points_out``: (batch, m) int32, the source point behind every point of the
    last launch (-1 beyond the length); ``expected_points`` restates them on the host."""

    FIELDS = ("func_in", "target", "mesh_in", "mesh_out", "len_in", "len_out")

    def __init__(self, step, data, shuffle: bool = True, seed: int = 0, drop_last: bool = True, rank: Optional[int] = None,
                 world_size: Optional[int] = None, order=None, subsample: bool = False):
        if getattr(step, "graph", None) is not None:
            raise ValueError("DeviceFeed: this step has already been captured (its graph holds no feed launch); attach the feed first")
        if getattr(step, "_feed", None) is not None:
            raise ValueError("DeviceFeed: this step already has a feed")
        unknown = [name for name in data if name not in self.FIELDS]
        if unknown or not data:
            raise ValueError(f"DeviceFeed: unknown field name(s) {unknown}; the step's static buffers are {', '.join(self.FIELDS)}")
        try:
            step._check_mesh_update(data.get("mesh_in"), data.get("mesh_out"))
        except ValueError as e:
            raise ValueError(f"DeviceFeed: {e}") from None
        self.subsample = bool(subsample)
        if self.subsample:
            if getattr(step, "affine", None) is not None:
                raise ValueError("DeviceFeed(subsample=True): a step with pred_affine - a per-pixel affine has no meaning on a "
                                 "subset of the points")
            if getattr(step, "pred", None) is not None:
                raise ValueError("DeviceFeed(subsample=True): EvalStep(store_pred=True) would store the predictions of another "
                                 "subset of the points in every pass")
        for name in ("len_in", "len_out"):
            if name in data and getattr(step, name) is None and not self.subsample:
                raise ValueError(f"DeviceFeed: field {name} on a step that was built without {name}")
        self.n_valid = getattr(step, "n_valid", None)
        if not drop_last and self.n_valid is None:
            raise ValueError(f"DeviceFeed: drop_last=False on a {type(step).__name__}: it has no n_valid, the samples that fill a "
                             "partly filled last batch would enter the loss")
        self.src, self.dst, self.names = [], [], []
        n = None
        one_cloud = self.subsample and (step.mesh_out is step.mesh_in or (step.mesh_out.data_ptr() == step.mesh_in.data_ptr()
                                                                           and step.mesh_out.shape == step.mesh_in.shape))
        self.kinds, self._widths = [], [None, None]                    # (subsample) per field its kind; per group (n_g, m_g)
        for name in self.FIELDS:
            if name not in data or (self.subsample and name in ("len_in", "len_out")):
                continue
            t, static = data[name], getattr(step, name)
            if not torch.is_tensor(t) or t.dim() < 1 or t.shape[0] < 1:
                raise ValueError(f"DeviceFeed: field {name} must be a tensor with a leading sample axis")
            if not static.is_contiguous() or not t.is_contiguous():
                raise ValueError(f"DeviceFeed: field {name} and its static buffer must be contiguous")
            if self.subsample:
                group = 0 if one_cloud or name in ("mesh_in", "func_in") else 1
                mesh = ("mesh_in", "mesh_out") if one_cloud else (("mesh_in",), ("mesh_out",))[group]
                if not any(k in data for k in mesh):
                    raise ValueError(f"DeviceFeed(subsample=True): point field {name} without {mesh[0]} in data - the subset of "
                                     "the function's points must be the subset of the mesh's")
                if t.dim() < 2 or t.dim() != static.dim() or t.dtype != static.dtype or t.shape[2:] != static.shape[2:] \
                        or t.device != static.device:
                    raise ValueError(f"DeviceFeed: field {name} has points {tuple(t.shape[2:])} {t.dtype} on {t.device}, the "
                                     f"step's static buffer {tuple(static.shape[2:])} {static.dtype} on {static.device}")
                if t.shape[1] < static.shape[1]:
                    raise ValueError(f"DeviceFeed(subsample=True): field {name} has {t.shape[1]} points, narrower than the step's "
                                     f"{static.shape[1]}")
                width = (int(t.shape[1]), int(static.shape[1]))
                if self._widths[group] not in (None, width):
                    raise ValueError(f"DeviceFeed(subsample=True): field {name} has {width[0]} points against the step's "
                                     f"{width[1]}, the fields of its cloud before it {self._widths[group][0]} against "
                                     f"{self._widths[group][1]}")
                if (static[0, 0].numel() * static.element_size()) % 4 or static[0, 0].numel() == 0:
                    raise ValueError(f"DeviceFeed: field {name}: points are copied as whole 4-byte words")
            elif t.dtype != static.dtype or t.shape[1:] != static.shape[1:] or t.device != static.device:
                raise ValueError(f"DeviceFeed: field {name} has rows {tuple(t.shape[1:])} {t.dtype} on {t.device}, the step's static "
                                 f"buffer {tuple(static.shape[1:])} {static.dtype} on {static.device}")
            if (static[0].numel() * static.element_size()) % 4 or static[0].numel() == 0:
                raise ValueError(f"DeviceFeed: field {name}: rows are copied as whole 4-byte words")
            if n is not None and t.shape[0] != n:
                raise ValueError(f"DeviceFeed: field {name} has {t.shape[0]} samples, the fields before it {n}")
            n = t.shape[0]
            shared = [k for k, d in enumerate(self.dst) if static.data_ptr() == d.data_ptr()]
            if shared:                                                 # shares its static buffer with a field already taken
                if t.data_ptr() != self.src[shared[0]].data_ptr():
                    raise ValueError(f"DeviceFeed: {name} and {self.names[shared[0]]} share one static buffer of the step but "
                                     "bring different data; pass the same tensor for both (or one of them)")
                continue
            self.src.append(t)
            self.dst.append(static)
            self.names.append(name)
            if self.subsample:
                self.kinds.append(1 + group)
                self._widths[group] = width
        if len(self.src) > 8:
            raise ValueError("DeviceFeed: at most 8 fields")
        if self.subsample and not self.src:
            raise ValueError("DeviceFeed(subsample=True): data holds lengths only")
        if rank is None or world_size is None:
            import torch.distributed as dist
            up = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if up else 0) if rank is None else rank
            world_size = (dist.get_world_size() if up else 1) if world_size is None else world_size
        self.rank, self.world_size = int(rank), int(world_size)
        if self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError(f"DeviceFeed: rank {self.rank} outside [0, {self.world_size})")
        self.n_samples, self.batch = int(n), int(self.dst[0].shape[0])
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        per_step = self.batch * self.world_size
        if self.drop_last and self.n_samples < per_step:
            raise ValueError(f"DeviceFeed: drop_last with {self.n_samples} samples and {per_step} per step leaves no full step")
        self.steps_per_epoch = self.n_samples // per_step if self.drop_last else -(-self.n_samples // per_step)
        dev = self.dst[0].device
        self.order = None
        if order is not None:
            order = torch.as_tensor(order)
            if order.dim() != 1 or order.numel() != self.n_samples or order.is_floating_point():
                raise ValueError(f"DeviceFeed: order must hold {self.n_samples} integer sample indices")
            lim = torch.iinfo(torch.int32)
            self.order = order.detach().to(torch.int64).clamp(lim.min, lim.max).to(device=dev, dtype=torch.int32).contiguous()
        self._host_order = None                                        # (a host copy of ``order``, made by expected_indices)
        self.state = ops.new_feed_state(dev)                           # the cursor and the arrival ticket
        self.cursor = self.state[0]
        self.indices = torch.zeros(self.batch, device=dev, dtype=torch.int32)
        self.points_in = self.points_out = None
        if self.subsample:
            self._init_subsample(step, data, one_cloud, dev)
        self.step = step
        step._feed = self

    def _init_subsample(self, step, data, one_cloud: bool, dev) -> None:
        """The source lengths, the static lengths the launch writes and the index tables of a subsampling feed."""
        self._len_src, self._len_dst, self._host_len = [None, None], [None, None], [None, None]
        for g, name in enumerate(("len_in", "len_out")):
            lengths, static = data.get(name), getattr(step, name)
            if g == 1 and one_cloud and (lengths is not None or static is not None):
                raise ValueError("DeviceFeed(subsample=True): len_out on a step whose mesh_out is its mesh_in - the one cloud has "
                                 "one length, len_in")
            if self._widths[g] is None:
                if lengths is not None:
                    raise ValueError(f"DeviceFeed(subsample=True): {name} without a point field of its cloud in data")
                continue
            n_g, m_g = self._widths[g]
            if lengths is not None:
                if not torch.is_tensor(lengths) or lengths.shape != (self.n_samples,) or lengths.is_floating_point() \
                        or lengths.device != dev:
                    raise ValueError(f"DeviceFeed: field {name} must hold {self.n_samples} integer lengths on {dev}")
                if static is None:
                    # a rectangular step: every cloud must fill it (one read of the lengths, here and never again)
                    shortest = int(lengths.clamp(1, n_g).min())
                    if shortest < m_g:
                        raise ValueError(f"DeviceFeed(subsample=True): the shortest cloud of {name} has {shortest} points, the "
                                         f"step takes {m_g}; build the step with {name}= (it then receives min({m_g}, length) "
                                         "points per sample) or with fewer points")
                self._len_src[g] = lengths.to(torch.int32).contiguous()
            self._len_dst[g] = static
            table = torch.full((self.batch, m_g), -1, device=dev, dtype=torch.int32)
            if g == 0:
                self.points_in = table
            else:
                self.points_out = table
        self.n_in, self.m_in = self._widths[0] or (0, 0)
        self.n_out, self.m_out = self._widths[1] or (0, 0)

    def seek(self, k: int) -> None:
        """The next launch is feed number ``k`` (epoch k // steps_per_epoch, step k % steps_per_epoch): a device fill, no
        synchronisation."""
        if int(k) < 0:
            raise ValueError("seek: a feed position is not negative")
        self.cursor.fill_(int(k))

    _STATE_KEYS = ("n_samples", "batch", "world_size", "seed", "shuffle", "drop_last", "steps_per_epoch")

    _SUBSAMPLE_KEYS = ("subsample", "n_in", "m_in", "n_out", "m_out")

    def _state_keys(self):
        return self._STATE_KEYS + (self._SUBSAMPLE_KEYS if self.subsample else ())

    def state_dict(self) -> dict:
        """The feed's position - ``cursor``, the number of feeds so far (one device->host read) - and what gives it its meaning:
        n_samples, batch, world_size, seed, shuffle, drop_last and steps_per_epoch, as plain numbers.  A caller-supplied
        ``order`` is NOT saved: a run that resumes with another ``order`` reads other samples at the same position.  A
        subsampling feed adds ``subsample`` and the source and destination widths of its clouds (n_in, m_in, n_out, m_out; 0
        for a cloud it does not feed): the subsets are a function of (seed, epoch, sample, group), so the position is all a
        resumed run needs to draw the same ones."""
        state = {"cursor": int(self.cursor)}
        state.update({key: getattr(self, key) for key in self._state_keys()})
        return state

    def load_state_dict(self, state: dict) -> None:
        """``seek(state["cursor"])``, after checking that this feed is the one the position was saved from: a different
        n_samples, batch, world_size, seed, shuffle, drop_last or steps_per_epoch raises ValueError (the position would mean
        other samples).  So does a state saved with ``subsample`` loaded into a feed without, or the reverse, or with other
        widths."""
        if bool(state.get("subsample", False)) != self.subsample:
            raise ValueError(f"DeviceFeed.load_state_dict: the state was saved with subsample = {bool(state.get('subsample', False))!r}, "
                             f"this feed has subsample = {self.subsample!r}: the position would mean other points")
        for key in self._state_keys():
            if key not in state or state[key] != getattr(self, key):
                raise ValueError(f"DeviceFeed.load_state_dict: the state was saved with {key} = {state.get(key)!r}, this feed "
                                 f"has {key} = {getattr(self, key)!r}: the position would mean other samples")
        self.seek(state["cursor"])

    def launch(self) -> None:
        """One feed, eagerly (the steps call this as the first launch of their ``_step``)."""
        if self.subsample:
            ops.batch_feed_points(self.src, self.dst, self.kinds, self.state, self.rank, self.world_size, self.drop_last,
                                  self.shuffle, self.order, self.seed, self.indices, self.n_valid, self._len_src, self._len_dst,
                                  (self.points_in, self.points_out))
            return
        ops.batch_feed(self.src, self.dst, self.state, self.rank, self.world_size, self.drop_last, self.shuffle, self.order,
                       self.seed, self.indices, self.n_valid)

    def expected_indices(self, cursor: int):
        """(the sample index behind every slot, n_valid) of the launch at ``cursor`` for this rank, restated on the host
        (``feed_order``); reads ``order`` back once when the feed has one."""
        n, c = self.n_samples, max(int(cursor), 0)
        epoch, i = divmod(c, self.steps_per_epoch)
        first = (i * self.world_size + self.rank) * self.batch
        pos = [(first + s) % n for s in range(self.batch)]
        if self.order is not None:
            if self._host_order is None:
                self._host_order = self.order.cpu().tolist()
            idx = [min(max(self._host_order[g], 0), n - 1) for g in pos]
        elif not self.shuffle:
            idx = pos
        else:
            perm = feed_order(n, self.seed, epoch)
            idx = [int(perm[g]) for g in pos]
        return idx, min(max(n - first, 0), self.batch)

    def expected_points(self, cursor: int):
        """``(points_in, points_out)`` of the launch at ``cursor`` for this rank, restated on the host: per group a list with,
        for every slot, the LongTensor of source points that arrive (``feed_points`` for the slot's sample of
        ``expected_indices``, with host copies of the source lengths, read back once); None for a group the feed does not
        have.  Slot s of the launch holds ``src[idx][points]`` in its first ``len(points)`` rows and zeros beyond."""
        if not self.subsample:
            raise ValueError("expected_points: this feed was built without subsample")
        idx, _ = self.expected_indices(cursor)
        epoch = max(int(cursor), 0) // self.steps_per_epoch
        out = []
        for g in range(2):
            if self._widths[g] is None:
                out.append(None)
                continue
            n_g, m_g = self._widths[g]
            if self._len_src[g] is not None and self._host_len[g] is None:
                self._host_len[g] = self._len_src[g].cpu().tolist()
            lens = self._host_len[g]
            out.append([feed_points(min(max(lens[i], 1), n_g) if lens is not None else n_g, m_g, self.seed, epoch, i, g)
                        for i in idx])
        return tuple(out)
