"""GPU: averaged weights in the guarded step (ddp.AveragedAdam over pit_adam_step_averaged), the in-place exchange behind their
evaluation (pit_exchange_words) and the exact resume of a captured run (engine.TrainStep.state_dict / load_state_dict).

Sizes come from the launch code (csrc/pit_optim.hip).  The update's grid-stride loop wraps above 2048 * 256 = 524 288 elements
(524 365 takes a second trip), a norm partial covers 1024 * ceil(n / 262 144) elements (262 147: the run doubles), 1023 / 1025
sit on either side of one partial, 1 and 37 are a ragged single workgroup.  The exchange moves 16-byte groups of four words with
up to three single head and tail words: 1, 3 (no group), 1023, 1024, 1025 (tails of 3, 0, 1; with a head of 3: 0, 1, 2) and
2 097 157 = 4 * 2048 * 256 + 5 (the group loop's second trip).

Bounds.  Everything is compared as bits except the second check of the average: against the fp64 recurrence
a += w * (p - a) with the fp64 weight, within 8 * 2^-24 * M * min(K, 1 / (1 - d)) (K alone in equal mode) - three fp32
roundings per update (the difference, the product, the sum; each at most 2^-24 relative of a value no larger than 2 M), and one
more for the weight's own rounding to fp32, contracted by d per update; M is the largest magnitude seen, K the number of
averaged updates.  An fp32 emulation of six updates on the CPU (200 000 normal values) reaches 11 % of it at the first
averaged update (K = 1) and less afterwards; the test prints the kernel's largest share (on MI355X: 0.03 .. 0.11)."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_guard import T_MAX, WD, _bits, _gradients, _optimizer, _same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 37, 1023, 1025, 262147, 524365]
GUARD_KW = dict(weight_decay=WD, cosine_t_max=T_MAX, zero_grads=True, max_grad_norm=0.5, decoupled=True, warmup_steps=2,
                warmup_start=0.1)


def _gradient_list(n, calls):
    """``calls`` gradients of n elements and the starting parameters (test_gpu_guard's generator, one more draw when needed)."""
    p0, grads, _ = _gradients(n)
    g = torch.Generator().manual_seed(n + 77)
    while len(grads) < calls:
        grads.append(torch.randn(n, generator=g) * 0.5)
    return p0, grads[:calls]


# --------------------------------------------------------------------------- the average does not touch the step
@pytest.mark.parametrize("n", SIZES)
def test_averaged_step_has_the_guarded_steps_bits(n):
    from position_induced_transformer_amd.ddp import AveragedAdam, GuardedAdam
    p0, grads = _gradient_list(n, 4)
    guarded, flat_a = _optimizer(GuardedAdam, p0, n, **GUARD_KW)
    averaged, flat_b = _optimizer(AveragedAdam, p0, n, average="ema", average_decay=0.9, **GUARD_KW)
    assert averaged.average.numel() == n
    for call, grad in enumerate(grads, start=1):
        for opt, flat in ((guarded, flat_a), (averaged, flat_b)):
            flat.flat.copy_(grad.cuda())
            opt.step()
        for name in ("exp_avg", "exp_avg_sq", "step_count", "calls", "state", "scalars"):
            assert _same_bits(getattr(guarded, name), getattr(averaged, name)), (call, name)
        assert _same_bits(flat_a.flat_params, flat_b.flat_params), call
        assert _same_bits(flat_a.flat, flat_b.flat) and not bool(_bits(flat_b.flat).any())
        assert int(averaged.step_count) == int(averaged.calls) == int(averaged.n_averaged) == call
        assert int(_bits(averaged.scalars)[3]) == 0                   # the ticket word
    health = averaged.health()
    assert (health.calls, health.applied, health.skipped) == (4, 4, 0) and health.clipped >= 1
    assert not _same_bits(averaged.average, flat_b.flat_params)       # an average, not a copy


# --------------------------------------------------------------------------- the average itself
MODES = {
    "ema0.9": dict(average="ema", average_decay=0.9),
    "ema0.999-ramp": dict(average="ema", average_decay=0.999, average_ramp=True),
    "equal": dict(average="equal"),
    "ema0.9-start2": dict(average="ema", average_decay=0.9, average_start=2),
}


class _Restated:
    """The header's rule on the CPU: in fp32, operation by operation (``a32``), and as an fp64 recurrence (``a64``)."""

    def __init__(self, p0, average="ema", average_decay=0.999, average_ramp=False, average_start=0):
        self.mode, self.decay, self.ramp, self.start = average, average_decay, average_ramp, average_start
        self.a32, self.a64 = p0.clone(), p0.double()
        self.applied, self.largest = 0, float(p0.abs().max())

    @property
    def averaged(self):
        return max(0, self.applied - self.start)

    def update(self, p):
        from position_induced_transformer_amd.ddp import average_weight
        self.applied += 1
        self.largest = max(self.largest, float(p.abs().max()))
        m = self.applied - self.start
        if m < 1:
            self.a32, self.a64 = p.clone(), p.double()
            return
        w = average_weight(m, self.mode, self.decay, self.ramp)
        w32 = np.float32(w)
        if w32 == np.float32(1.0):
            self.a32 = p.clone()
        else:
            diff = p - self.a32                                       # three tensor operations, each rounded to fp32
            prod = diff * torch.tensor(w32)
            self.a32 = self.a32 + prod
        self.a64 = self.a64 + w * (p.double() - self.a64)
        self.largest = max(self.largest, float(self.a64.abs().max()))

    def bound(self):
        k = self.averaged
        if self.mode == "ema":
            k = min(k, 1.0 / (1.0 - self.decay))
        return 8.0 * 2.0 ** -24 * self.largest * k


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_average_equals_its_fp32_restatement_as_bits(n, mode):
    from position_induced_transformer_amd.ddp import AveragedAdam
    p0, grads = _gradient_list(n, 6)
    opt, flat = _optimizer(AveragedAdam, p0, n, **MODES[mode], **GUARD_KW)
    want = _Restated(p0, **MODES[mode])
    assert _same_bits(opt.average.cpu(), p0) and int(opt.n_averaged) == 0
    worst = 0.0
    for call, grad in enumerate(grads, start=1):
        flat.flat.copy_(grad.cuda())
        opt.step()
        p = flat.flat_params.cpu()
        want.update(p)
        got = opt.average.cpu()
        assert torch.isfinite(got).all()
        assert _same_bits(got, want.a32), (call, int((_bits(got) != _bits(want.a32)).sum()))
        err, bound = float((got.double() - want.a64).abs().max()), want.bound()
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (call, err, bound)
        assert int(opt.n_averaged) == want.averaged == max(0, call - MODES[mode].get("average_start", 0))
        assert opt.health().applied == call
    print("average %s n=%d: largest distance from the fp64 recurrence %.3f of its bound" % (mode, n, worst))


# --------------------------------------------------------------------------- a skipped call
@pytest.mark.parametrize("mode", ["equal", "ema0.999-ramp"])
@pytest.mark.parametrize("n", [37, 262147, 524365])
def test_a_skipped_call_leaves_the_average_alone(n, mode):
    """A NaN gradient in call 3 of 5 (in the update grid's second trip where there is one): average and n_averaged keep the bits
    of call 2, and call 4 is averaged update m = 3 - both modes' weights depend on m."""
    from position_induced_transformer_amd.ddp import AveragedAdam
    p0, grads = _gradient_list(n, 5)
    opt, flat = _optimizer(AveragedAdam, p0, n, **MODES[mode], **GUARD_KW)
    want = _Restated(p0, **MODES[mode])
    for call, grad in enumerate(grads, start=1):
        grad = grad.clone()
        if call == 3:
            grad[n - 1] = float("nan")
        before = [t.clone() for t in (opt.average, opt.n_averaged, flat.flat_params)]
        flat.flat.copy_(grad.cuda())
        opt.step()
        if call == 3:
            assert all(_same_bits(a, b) for a, b in zip(before, (opt.average, opt.n_averaged, flat.flat_params)))
            assert int(opt.n_averaged) == 2 and opt.health().skipped == 1
        else:
            want.update(flat.flat_params.cpu())
            assert _same_bits(opt.average.cpu(), want.a32), call
            assert int(opt.n_averaged) == want.averaged == call - (call > 3)
        assert int(opt.calls) == call and not bool(_bits(flat.flat).any())
    assert want.averaged == 4 and torch.isfinite(opt.average).all()


# --------------------------------------------------------------------------- the exchange
WORDS = [1, 3, 1023, 1024, 1025, 2097157]
NAN_WORDS = [0x7FC00001, 0x7F800001, -0x3EDCBB, -0x7FFFFF, 0x7FFFFFFF, -1]      # quiet, signalling and negative NaNs with payloads
GUARD = 4


def _room(n, offset, seed, salt=0):
    """An int32 allocation with GUARD + offset words in front of the n-word view and GUARD behind it; the view's base is
    16-byte aligned for offset 0 and 4 * offset bytes past a boundary otherwise.  ``salt`` changes the payloads of the NaN
    words planted in the view (the two sides of an exchange must differ in every one of them)."""
    g = torch.Generator().manual_seed(seed)
    host = torch.randint(-2 ** 31, 2 ** 31 - 1, (GUARD + offset + n + GUARD,), generator=g, dtype=torch.int64).to(torch.int32)
    first = GUARD + offset
    for k, word in enumerate(NAN_WORDS):                              # NaN patterns at both ends and inside
        host[first + (k * max(n // len(NAN_WORDS), 1)) % n] = word ^ salt
    host[first + n - 1] = NAN_WORDS[0] ^ salt
    room = host.cuda()
    view = room[first:first + n]
    assert room.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * offset
    return host, room, view, first


@pytest.mark.parametrize("offsets", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["aligned", "a+1", "b+1", "both+1"])
@pytest.mark.parametrize("n", WORDS)
def test_exchange_words_swaps_raw_bits_and_nothing_else(n, offsets):
    from position_induced_transformer_amd import _lib
    host_a, room_a, a, first_a = _room(n, offsets[0], 2 * n)
    host_b, room_b, b, first_b = _room(n, offsets[1], 2 * n + 1, salt=0x2A)
    assert not torch.equal(host_a[first_a:first_a + n], host_b[first_b:first_b + n])
    fn = _lib.lib().pit_exchange_words
    for call in (1, 2):
        _lib.check(fn(a.data_ptr(), b.data_ptr(), n, _lib.stream_ptr()), "pit_exchange_words")
        got_a, got_b = room_a.cpu(), room_b.cpu()
        want_a, want_b = host_a.clone(), host_b.clone()
        if call == 1:                                                 # exchanged; after the second call: restored
            want_a[first_a:first_a + n] = host_b[first_b:first_b + n]
            want_b[first_b:first_b + n] = host_a[first_a:first_a + n]
        assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b), (call, n, offsets)      # the guard words included


# --------------------------------------------------------------------------- swap and evaluate
def _darcy_like(seed):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    return tasks.pit_darcy(2, 1, 1, 32, 2, 2, tasks.grid_mesh_2d(8, True, "cuda"), 0.05, 0.05).cuda()


def _darcy_data(n, seed=31):
    from position_induced_transformer_amd import tasks
    g = torch.Generator().manual_seed(seed)
    mesh = tasks.grid_mesh_2d(16, True).cuda()
    return mesh, torch.randn(n, 16, 16, 1, generator=g).cuda(), torch.randn(n, 16, 16, 1, generator=g).cuda()


def test_a_captured_eval_step_evaluates_the_swapped_in_average():
    """The tolerance is tests/test_gpu_eval_step.py's for replay against eager: the same launches run, so equality."""
    from position_induced_transformer_amd import ops, utils
    from position_induced_transformer_amd.ddp import AveragedAdam, FlatGradients
    from position_induced_transformer_amd.engine import EvalStep, TrainStep
    assert ops.get_head_scale_route() == "device"
    model = _darcy_like(7)
    mesh, x, y = _darcy_data(6)
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = AveragedAdam(flat, lr=1e-2, zero_grads=True, max_grad_norm=0.5, average="ema", average_decay=0.9)
    train = TrainStep(model, (mesh, x[:3].clone(), mesh, y[:3].clone()), 1, 2, optimizer=opt, flat=flat)
    ev = EvalStep(model, (mesh, x[3:].clone(), mesh, y[3:].clone()), 1, 2, capacity=3)
    train.capture()
    ev.capture()
    for _ in range(5):
        train.replay()
    assert int(opt.n_averaged) == int(opt.step_count) == 8            # three warm-up passes and five replays
    ev.reset(); ev.replay()
    live = ev.result()
    before, before_avg = flat.flat_params.clone(), opt.average.clone()
    assert not _same_bits(before, before_avg)
    with opt.averaged() as inside:
        assert inside is opt and opt.swapped
        assert _same_bits(flat.flat_params, before_avg) and _same_bits(opt.average, before)
        ev.reset(); ev.replay()                                       # the graph captured above: no new capture
        averaged = ev.result()
        out = ev.out.clone()
    assert not opt.swapped and _same_bits(flat.flat_params, before) and _same_bits(opt.average, before_avg)
    # the reference: an eager forward of a copy of the model that carries the averaged weights
    state = opt.averaged_model_state(model)
    assert list(state) == list(model.state_dict())
    twin = copy.deepcopy(model)
    twin.load_state_dict(state, strict=True)
    utils.load_reference_checkpoint(twin, {"model_state": state})
    eager = EvalStep(twin, (mesh, x[3:].clone(), mesh, y[3:].clone()), 1, 2, capacity=3)
    eager.reset(); eager.run_eager()
    want = eager.result()
    print("rel_lp live %.9g averaged %.9g eager on the averaged copy %.9g" % (live.rel_lp, averaged.rel_lp, want.rel_lp))
    assert averaged.count == want.count == 3 and math.isfinite(want.rel_lp)
    assert averaged.rel_lp == want.rel_lp and torch.equal(out, eager.out)
    assert averaged.rel_lp != live.rel_lp                             # it was the average that was evaluated
    # an exception inside the block swaps back too
    with pytest.raises(KeyError):
        with opt.averaged():
            raise KeyError("x")
    assert not opt.swapped and _same_bits(flat.flat_params, before) and _same_bits(opt.average, before_avg)
    train.replay()                                                    # and training goes on
    assert int(opt.n_averaged) == 9


# --------------------------------------------------------------------------- exact resume
def _resumable_run(model_seed):
    from position_induced_transformer_amd.ddp import AveragedAdam, FlatGradients
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    model = _darcy_like(model_seed)
    mesh, x, y = _darcy_data(24, seed=41)
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = AveragedAdam(flat, lr=1e-3, cosine_t_max=12, zero_grads=True, max_grad_norm=0.5, warmup_steps=2, warmup_start=0.1,
                       average="ema", average_decay=0.9)
    step = TrainStep(model, (mesh, x[:4].clone(), mesh, y[:4].clone()), 1, 2, optimizer=opt, flat=flat)
    feed = DeviceFeed(step, {"func_in": x, "target": y}, shuffle=True, seed=3)
    assert feed.steps_per_epoch == 6
    step.capture()
    assert int(feed.cursor) == 0
    return step, opt, feed


def _everything(step, opt, feed):
    torch.cuda.synchronize()
    named = {"params": opt.flat.flat_params, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "average": opt.average,
             "step_count": opt.step_count, "calls": opt.calls, "n_averaged": opt.n_averaged, "health": opt.state,
             "cursor": feed.cursor, "indices": feed.indices, "loss": step.loss}
    named.update({"model." + k: v for k, v in step.model.state_dict().items()})
    return {k: v.detach().clone() for k, v in named.items()}


def test_a_saved_run_resumes_with_the_same_bits(tmp_path):
    """A: 7 replays (across the epoch boundary at 6).  B: 4 replays, saved.  C: another model, captured, loaded, 3 replays."""
    from position_induced_transformer_amd import ops
    path = os.path.join(tmp_path, "run.pt")
    with ops.reproducible():
        step, opt, feed = _resumable_run(9)
        for _ in range(7):
            step.replay()
        a = _everything(step, opt, feed)
        step, opt, feed = _resumable_run(9)
        for _ in range(4):
            step.replay()
        torch.save(step.state_dict(), path)
        # without the load: the same three replays end elsewhere
        step, opt, feed = _resumable_run(10)
        for _ in range(3):
            step.replay()
        d = _everything(step, opt, feed)
        # with it
        step, opt, feed = _resumable_run(10)
        addresses = [q.data_ptr() for q in step.model.parameters()]
        step.load_state_dict(torch.load(path, weights_only=True))
        assert [q.data_ptr() for q in step.model.parameters()] == addresses and int(feed.cursor) == 4
        for _ in range(3):
            step.replay()
        c = _everything(step, opt, feed)
    assert set(a) == set(c) and a["health"].numel() == 10
    for name in a:
        assert _same_bits(a[name], c[name]), name
    assert int(a["cursor"]) == 7 and int(a["calls"]) == 10 and int(a["n_averaged"]) == int(a["step_count"]) == 10
    assert a["indices"].tolist() == feed.expected_indices(6)[0]       # the first step of the second epoch
    assert torch.isfinite(a["params"]).all() and torch.isfinite(a["average"]).all() and math.isfinite(float(a["loss"]))
    for name in ("params", "exp_avg", "exp_avg_sq", "average", "calls", "cursor", "health", "indices"):
        assert not _same_bits(a[name], d[name]), name                 # the comparison above could not pass without the load
