"""No GPU: the guarded optimizer step (pit_adam_step_guarded, pit_adam_guard_parts) in header, binding and source list, its
refusals before any launch, the host restatements of its partition (ddp.guard_parts) and of its schedule (ddp.guarded_lr)
against torch's schedulers, and the host-side checks of ddp.GuardedAdam."""
import ctypes
import math
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h
SLOTS = ["CALLS", "APPLIED", "SKIPPED", "CLIPPED", "LAST_NORM", "MAX_NORM", "LAST_COEF", "LOSS_SUM", "LOSS_FINITE", "LOSS_NONFINITE"]


# ----------------------------------------------------------------------------- header, binding, sources
def test_header_binding_and_sources_agree_on_the_guarded_entries():
    from position_induced_transformer_amd import _lib, build, ddp
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_GUARDED_ADAM 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    assert int(re.search(r"^#define PIT_GUARD_MAX_PARTS (\d+)$", text, flags=re.M).group(1)) == _lib.GUARD_MAX_PARTS == 256
    assert int(re.search(r"^#define PIT_GUARD_STATE_DOUBLES (\d+)$", text, flags=re.M).group(1)) == _lib.GUARD_STATE_DOUBLES == len(SLOTS)
    for i, slot in enumerate(SLOTS):                                  # the state's layout is fixed in the header
        assert int(re.search(r"^#define PIT_GUARD_%s (\d+)\b" % slot, text, flags=re.M).group(1)) == i, slot
    assert ddp.GuardHealth._fields == ("calls", "applied", "skipped", "clipped", "norm", "max_norm", "coef", "loss_sum",
                                       "finite_loss", "nonfinite_loss", "mean_loss")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in (("pit_adam_guard_parts", 1), ("pit_adam_step_guarded", 24)):
        assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]) == count, name
        assert hasattr(_lib.lib(), name)
    assert "pit_optim.hip" in build.SOURCES
    source = open(os.path.join(build.CSRC, "pit_optim.hip")).read()
    assert "grad_sumsq_kernel" in source and "adam_step_guarded_kernel" in source
    assert _lib.lib().pit_version() == 31
    block = text[text.index("The guarded optimizer step"):text.index("#define PIT_HAS_GUARDED_ADAM")]
    assert "train_darcy.py:115-116,131-134" in block and "Beyond the reference" in block
    # the entry that existed keeps its declaration
    assert len(_lib.SIGNATURES["pit_adam_step"]) == 16


# ----------------------------------------------------------------------------- refusals before any launch
_buf = (ctypes.c_longlong * 64)()
P = ctypes.addressof(_buf)

BASE = dict(params=P, grads=P, exp_avg=P, exp_avg_sq=P, n=37, step=P, calls=P, lr0=1e-3, eta_min=0.0, cosine_t_max=10,
            warmup_steps=3, warmup_start=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, max_norm=1.0,
            zero_grads=1, loss=None, partials=P, state=P, scalars=P, stream=None)

TABLE = [
    (dict(params=None), NULL),
    (dict(grads=None), NULL),
    (dict(exp_avg=None), NULL),
    (dict(exp_avg_sq=None), NULL),
    (dict(step=None), NULL),
    (dict(calls=None), NULL),
    (dict(partials=None), NULL),
    (dict(state=None), NULL),
    (dict(scalars=None), NULL),
    (dict(n=0), SIZE),
    (dict(n=-5), SIZE),
    (dict(grads=P + 2), SIZE),                                        # gradients are read as aligned words
    (dict(max_norm=-1.0), UNSUPPORTED),
    (dict(max_norm=-1e-300), UNSUPPORTED),
    (dict(max_norm=float("nan")), UNSUPPORTED),
    (dict(warmup_steps=-1), UNSUPPORTED),
    (dict(warmup_start=-0.1), UNSUPPORTED),
    (dict(warmup_start=1.5), UNSUPPORTED),
    (dict(warmup_start=float("nan")), UNSUPPORTED),
    (dict(params=None, n=0, max_norm=-1.0), NULL),                    # the order of the checks: pointers, sizes, values
    (dict(n=0, max_norm=-1.0), SIZE),
]


def test_guarded_step_refuses_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    fn = _lib.lib().pit_adam_step_guarded
    assert list(BASE) == ["params", "grads", "exp_avg", "exp_avg_sq", "n", "step", "calls", "lr0", "eta_min", "cosine_t_max",
                          "warmup_steps", "warmup_start", "beta1", "beta2", "eps", "weight_decay", "decoupled", "max_norm",
                          "zero_grads", "loss", "partials", "state", "scalars", "stream"]
    assert len(BASE) == len(_lib.SIGNATURES["pit_adam_step_guarded"])        # the table's argument order is the header's
    for changed, code in TABLE:
        assert set(changed) <= set(BASE)
        assert fn(*{**BASE, **changed}.values()) == code, changed
    # a missing loss is no refusal: with it absent the call above is refused for nothing else
    assert BASE["loss"] is None and fn(*{**BASE, "n": 0}.values()) == SIZE
    assert not any(_buf)                                              # nothing was written through the host pointers
    parts = _lib.lib().pit_adam_guard_parts
    assert parts(0) == SIZE and parts(-1) == SIZE


# ----------------------------------------------------------------------------- the partition of the norm
@pytest.mark.parametrize("n", [1, 1024, 1025, 262144, 262145, 600001, (1 << 31) + 5])
def test_guard_parts_cover_the_buffer_exactly(n):
    from position_induced_transformer_amd import _lib
    from position_induced_transformer_amd.ddp import guard_parts, guard_run
    parts, run = guard_parts(n), guard_run(n)
    assert parts == _lib.lib().pit_adam_guard_parts(n)
    assert 1 <= parts <= 256
    assert run % 1024 == 0 and run == 1024 * -(-n // (1024 * 256))    # the length depends on n alone
    runs = [(b * run, min(n, (b + 1) * run)) for b in range(parts)]
    assert runs[0][0] == 0 and runs[-1][1] == n
    assert all(a < b for a, b in runs)                                # no empty run
    assert all(runs[i][1] == runs[i + 1][0] for i in range(parts - 1))       # no gap, no overlap
    want = {1: 1, 1024: 1, 1025: 2, 262144: 256, 262145: 129, 600001: 196}   # (262145: the run doubles to 2048)
    if n in want:
        assert parts == want[n]


def test_guard_parts_refuses_an_empty_buffer():
    from position_induced_transformer_amd.ddp import guard_parts
    with pytest.raises(ValueError, match="positive"):
        guard_parts(0)


# ----------------------------------------------------------------------------- the schedule
LR, ETA_MIN, T_MAX = 1e-3, 1e-5, 7


def _torch_rates(make_scheduler, steps):
    """The rate torch uses at each of ``steps`` optimizer steps, scheduler.step() after every one."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR)
    sched = make_scheduler(opt)
    rates = []
    for _ in range(steps):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return rates


@pytest.mark.parametrize("warmup,start,t_max", [(0, 0.0, T_MAX), (4, 0.0, T_MAX), (4, 0.25, T_MAX), (3, 1.0, 0), (0, 0.0, 0), (1, 0.5, 2)])
def test_guarded_lr_is_the_lambda_lr_of_its_closed_form(warmup, start, t_max):
    from position_induced_transformer_amd.ddp import guarded_lr

    def closed(k):                                                    # the header's two lines, written out again
        if k <= warmup:
            return LR * (start + (1.0 - start) * (k - 1) / warmup)
        if t_max > 0:
            return ETA_MIN + 0.5 * (LR - ETA_MIN) * (1.0 + math.cos(math.pi * (k - 1 - warmup) / t_max))
        return LR

    steps = warmup + 2 * max(t_max, 1) + 3
    rates = _torch_rates(lambda opt: torch.optim.lr_scheduler.LambdaLR(opt, lambda e: closed(e + 1) / LR), steps)
    for k, want in enumerate(rates, start=1):
        got = guarded_lr(k, LR, ETA_MIN, t_max, warmup, start)
        assert abs(got - want) <= 4e-16 * LR, (k, got, want)          # LambdaLR: one division and one product in fp64
    if warmup:
        assert guarded_lr(1, LR, ETA_MIN, t_max, warmup, start) == LR * start
        assert guarded_lr(warmup + 1, LR, ETA_MIN, t_max, warmup, start) == LR        # the warm-up ends on the full rate
    with pytest.raises(ValueError, match="counted from 1"):
        guarded_lr(0, LR)


def test_guarded_lr_without_warmup_is_cosine_annealing_lr():
    from position_induced_transformer_amd.ddp import guarded_lr
    steps = 2 * T_MAX + 3                                             # through the minimum and back up
    rates = _torch_rates(lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_MAX, eta_min=ETA_MIN), steps)
    for k, want in enumerate(rates, start=1):
        # torch's recursive form drifts from the closed form by a rounding of LR per step
        assert abs(guarded_lr(k, LR, ETA_MIN, T_MAX) - want) <= steps * 2.3e-16 * LR, (k, want)


@pytest.mark.parametrize("warmup,start", [(5, 0.1), (1, 0.5), (8, 1.0)])
def test_guarded_lr_warmup_is_linear_lr(warmup, start):
    from position_induced_transformer_amd.ddp import guarded_lr
    rates = _torch_rates(lambda opt: torch.optim.lr_scheduler.LinearLR(opt, start_factor=start, total_iters=warmup), warmup + 1)
    for k, want in enumerate(rates, start=1):
        got = guarded_lr(k, LR, ETA_MIN, T_MAX, warmup, start)
        assert abs(got - want) <= (warmup + 1) * 2.3e-16 * LR, (k, got, want)          # (LinearLR is recursive too)


# ----------------------------------------------------------------------------- ddp.GuardedAdam on the host
def _flat(flatten=True):
    from position_induced_transformer_amd.ddp import FlatGradients
    return FlatGradients([torch.nn.Parameter(torch.zeros(5, 3))], flatten_params=flatten)


def test_guarded_adam_constructor():
    import inspect
    from position_induced_transformer_amd.ddp import FlatAdam, GuardedAdam
    assert issubclass(GuardedAdam, FlatAdam)
    assert list(inspect.signature(GuardedAdam.__init__).parameters)[1:] == [
        "flat", "lr", "betas", "eps", "weight_decay", "cosine_t_max", "eta_min", "zero_grads", "max_grad_norm", "decoupled",
        "warmup_steps", "warmup_start"]
    assert list(inspect.signature(FlatAdam.__init__).parameters)[1:] == [
        "flat", "lr", "betas", "eps", "weight_decay", "cosine_t_max", "eta_min", "zero_grads"]       # untouched
    opt = GuardedAdam(_flat(), max_grad_norm=2.5, decoupled=True, warmup_steps=4, warmup_start=0.5, zero_grads=True)
    assert opt.max_grad_norm == 2.5 and opt.decoupled and opt.warmup_steps == 4 and opt.warmup_start == 0.5 and opt.zero_grads
    assert opt.partials.dtype == torch.float64 and opt.partials.numel() == 256
    assert opt.state.dtype == torch.float64 and opt.state.numel() == len(SLOTS) and not opt.state.any()
    assert opt.calls.dtype == torch.int64 and int(opt.calls) == 0 and int(opt.step_count) == 0
    assert GuardedAdam(_flat()).max_grad_norm == 0.0                  # None: clipping is off
    health = opt.health()
    assert health.calls == health.skipped == health.finite_loss == 0 and math.isnan(health.mean_loss)


@pytest.mark.parametrize("kw,match", [
    (dict(max_grad_norm=-1.0), "max_grad_norm"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm"),
    (dict(warmup_steps=-1), "warmup_steps"),
    (dict(warmup_steps=2.5), "warmup_steps"),
    (dict(warmup_start=-0.01), "warmup_start"),
    (dict(warmup_start=1.01), "warmup_start"),
    (dict(warmup_start=float("nan")), "warmup_start"),
])
def test_guarded_adam_refuses_bad_arguments_on_the_host(kw, match):
    from position_induced_transformer_amd.ddp import GuardedAdam
    with pytest.raises(ValueError, match=match):
        GuardedAdam(_flat(), **kw)


def test_guarded_adam_needs_flat_parameters_and_an_fp32_scalar_loss():
    from position_induced_transformer_amd.ddp import GuardedAdam
    with pytest.raises(ValueError, match="flatten_params=True"):
        GuardedAdam(_flat(flatten=False))
    opt = GuardedAdam(_flat())
    opt.watch_loss(torch.zeros(()))
    opt.watch_loss(None)
    with pytest.raises(ValueError, match="fp32 scalar"):
        opt.watch_loss(torch.zeros((), dtype=torch.float64))
    with pytest.raises(ValueError, match="fp32 scalar"):
        opt.watch_loss(torch.zeros(2))


def test_train_step_health_forwards_to_the_optimizer():
    from position_induced_transformer_amd import pit as P_
    from position_induced_transformer_amd.engine import RolloutStep, TrainStep
    torch.manual_seed(0)
    model = P_.pit_fixed(2, 1, 1, 16, 2, 4, torch.rand(16, 2), 0.1, 0.1)
    mesh, x = torch.rand(36, 2), torch.zeros(8, 36, 1)

    class _Opt:
        def health(self, reset=False):
            return ("health", reset)

    step = TrainStep(model, (mesh, x, mesh, x.clone()), 1, 2, optimizer=_Opt())
    assert step.health() == ("health", False) and step.health(reset=True) == ("health", True)
    with pytest.raises(RuntimeError, match="GuardedAdam"):
        TrainStep(model, (mesh, x, mesh, x.clone()), 1, 2).health()
    assert RolloutStep._optimizer_step is TrainStep._optimizer_step   # the rollout hands its loss over the same way
