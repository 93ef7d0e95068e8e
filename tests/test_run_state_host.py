"""No GPU: averaged weights and the saved state of a captured run - pit_adam_step_averaged and pit_exchange_words in header,
binding and library, their refusals before any launch, ddp.average_weight, the host side of ddp.AveragedAdam and of the
state_dict / load_state_dict pairs of the fused optimizers and of engine.DeviceFeed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h


# ----------------------------------------------------------------------------- header, binding, library
def test_header_binding_and_library_agree_on_the_new_entries():
    from position_induced_transformer_amd import _lib, build
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_AVERAGED_ADAM 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in (("pit_adam_step_averaged", 30), ("pit_exchange_words", 4), ("pit_adam_step_guarded", 24)):
        assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]) == count, name
        assert hasattr(_lib.lib(), name)
    # the averaged entry is the guarded one up to `scalars`, six arguments, then the stream
    guarded, averaged = _lib.SIGNATURES["pit_adam_step_guarded"], _lib.SIGNATURES["pit_adam_step_averaged"]
    assert averaged[:23] == guarded[:23] and averaged[-1] == guarded[-1]
    assert averaged[23:29] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_longlong]
    assert _lib.lib().pit_version() == 31
    block = text[text.index("Averaged weights in the guarded step"):text.index("#define PIT_HAS_AVERAGED_ADAM")]
    assert "train_darcy.py:150" in block and "Beyond the reference" in block
    source = open(os.path.join(build.CSRC, "pit_optim.hip")).read()
    assert "grad_sumsq_kernel" in source and "adam_step_guarded_kernel" in source and "exchange_words_kernel" in source


# ----------------------------------------------------------------------------- refusals before any launch
_buf = (ctypes.c_longlong * 64)()                                     # 512 bytes, 16-byte aligned or not: only differences matter
P = ctypes.addressof(_buf)
Q = P + 256                                                           # a second region: 37 floats from P end at P + 148

BASE = dict(params=P, grads=P, exp_avg=P, exp_avg_sq=P, n=37, step=P, calls=P, lr0=1e-3, eta_min=0.0, cosine_t_max=10,
            warmup_steps=3, warmup_start=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, max_norm=1.0,
            zero_grads=1, loss=None, partials=P, state=P, scalars=P, average=Q, n_averaged=P, avg_mode=0, avg_decay=0.9,
            avg_ramp=0, avg_start=0, stream=None)

# every case is a refusal: the accepted call would launch on host memory.  What each refusal rests on is shown by the case
# beside it that differs in one value and is refused for the NEXT reason in the order.
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
    (dict(average=None), NULL),
    (dict(n_averaged=None), NULL),
    (dict(n=0), SIZE),
    (dict(n=-5), SIZE),
    (dict(grads=P + 2), SIZE),
    (dict(max_norm=-1.0), UNSUPPORTED),                               # the guarded entry's value checks are kept
    (dict(max_norm=float("nan")), UNSUPPORTED),
    (dict(warmup_steps=-1), UNSUPPORTED),
    (dict(warmup_start=1.5), UNSUPPORTED),
    (dict(avg_mode=2), UNSUPPORTED),
    (dict(avg_mode=-1), UNSUPPORTED),
    (dict(avg_decay=1.0), UNSUPPORTED),                               # EMA: [0, 1)
    (dict(avg_decay=-1e-300), UNSUPPORTED),
    (dict(avg_decay=1.5), UNSUPPORTED),
    (dict(avg_decay=float("nan")), UNSUPPORTED),
    (dict(avg_start=-1), UNSUPPORTED),
    (dict(average=P), UNSUPPORTED),                                   # the average IS the parameters
    (dict(average=P + 4), UNSUPPORTED),                               # one element in
    (dict(average=P + 4 * 36), UNSUPPORTED),                          # the last element of params is the first of average
    (dict(params=Q + 4 * 36), UNSUPPORTED),                           # ... and the other way round
    (dict(average=None, n=0, avg_mode=7), NULL),                      # the order of the checks: pointers, sizes, values
    (dict(n_averaged=None, grads=P + 2), NULL),
    (dict(n=0, avg_mode=7), SIZE),
    (dict(grads=P + 2, avg_decay=2.0), SIZE),
    (dict(n=0, average=P), SIZE),
]


def test_averaged_step_refuses_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    fn = _lib.lib().pit_adam_step_averaged
    assert list(BASE) == ["params", "grads", "exp_avg", "exp_avg_sq", "n", "step", "calls", "lr0", "eta_min", "cosine_t_max",
                          "warmup_steps", "warmup_start", "beta1", "beta2", "eps", "weight_decay", "decoupled", "max_norm",
                          "zero_grads", "loss", "partials", "state", "scalars", "average", "n_averaged", "avg_mode", "avg_decay",
                          "avg_ramp", "avg_start", "stream"]
    assert len(BASE) == len(_lib.SIGNATURES["pit_adam_step_averaged"]) == 30
    for changed, code in TABLE:
        assert set(changed) <= set(BASE)
        assert fn(*{**BASE, **changed}.values()) == code, changed
    # equal mode does not look at the decay: with it out of range the call is refused for the overlap alone
    assert fn(*{**BASE, "avg_mode": 1, "avg_decay": 2.0, "average": P}.values()) == UNSUPPORTED
    assert fn(*{**BASE, "avg_mode": 1, "avg_decay": 2.0, "n": 0}.values()) == SIZE
    assert not any(_buf)                                              # nothing was written through the host pointers


EXCHANGE = [
    (dict(a=None), NULL),
    (dict(b=None), NULL),
    (dict(a=None, n_words=0), NULL),                                  # pointers first
    (dict(n_words=0), SIZE),
    (dict(n_words=-3), SIZE),
    (dict(a=P + 2), SIZE),
    (dict(b=Q + 1), SIZE),
    (dict(b=P, n_words=0), SIZE),                                     # sizes before the overlap
    (dict(b=P), UNSUPPORTED),                                         # a buffer with itself
    (dict(b=P + 4), UNSUPPORTED),                                     # b inside a's range
    (dict(b=P + 4 * 36), UNSUPPORTED),                                # a's last word is b's first
    (dict(a=Q, b=Q - 4 * 36), UNSUPPORTED),                           # b's last word is a's first
]


def test_exchange_refuses_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    fn = _lib.lib().pit_exchange_words
    base = dict(a=P, b=Q, n_words=37, stream=None)
    assert len(base) == len(_lib.SIGNATURES["pit_exchange_words"]) == 4
    for changed, code in EXCHANGE:
        assert fn(*{**base, **changed}.values()) == code, changed
    assert not any(_buf)


# ----------------------------------------------------------------------------- the weight of the average
def test_average_weight_ema_equal_and_ramp():
    from position_induced_transformer_amd.ddp import average_weight
    for decay in (0.0, 0.5, 0.9, 0.999):
        for m in (1, 2, 17, 10 ** 6):
            assert average_weight(m, "ema", decay) == 1.0 - decay
    for m in (1, 2, 3, 7, 1000, 10 ** 9):
        assert average_weight(m, "equal") == 1.0 / m
        assert average_weight(m, "equal", decay=0.3, ramp=True) == 1.0 / m        # (neither is looked at)
    assert average_weight(1, "equal") == 1.0 and np.float32(average_weight(1, "equal")) == np.float32(1.0)
    # the ramp: (1 + m) / (10 + m) reaches d at m = (10 d - 1) / (1 - d): 80 for 0.9, 8990 for 0.999
    for decay, crossing in ((0.9, 80), (0.999, 8990)):
        for m in list(range(1, 200)) + [crossing - 1, crossing, crossing + 1, 10 * crossing]:
            ramp = (1.0 + m) / (10.0 + m)
            w = average_weight(m, "ema", decay, ramp=True)
            if ramp < decay:
                assert w == 1.0 - ramp, (decay, m)
            else:
                assert w == 1.0 - decay, (decay, m)
        below, above = (1.0 + crossing - 1) / (10.0 + crossing - 1), (1.0 + crossing + 1) / (10.0 + crossing + 1)
        assert below < decay < above                                   # the crossing lies where the closed form puts it
        assert average_weight(crossing - 1, "ema", decay, ramp=True) == 1.0 - below > 1.0 - decay
        assert average_weight(crossing + 1, "ema", decay, ramp=True) == 1.0 - decay
    assert average_weight(1, "ema", 0.999, ramp=True) == 1.0 - 2.0 / 11.0
    for bad in (0, -1):
        with pytest.raises(ValueError, match="counted from 1"):
            average_weight(bad)
    with pytest.raises(ValueError, match="mode"):
        average_weight(1, "median")


# ----------------------------------------------------------------------------- ddp.AveragedAdam on the host
def _flat(rows=5):
    from position_induced_transformer_amd.ddp import FlatGradients
    torch.manual_seed(rows)
    return FlatGradients([torch.nn.Parameter(torch.randn(rows, 3))], flatten_params=True)


def test_averaged_adam_constructor():
    from position_induced_transformer_amd.ddp import AveragedAdam, FlatAdam, GuardedAdam
    assert issubclass(AveragedAdam, GuardedAdam)
    guarded = list(inspect.signature(GuardedAdam.__init__).parameters)
    assert list(inspect.signature(AveragedAdam.__init__).parameters) == guarded + ["average", "average_decay", "average_ramp",
                                                                                   "average_start"]
    defaults = {k: v.default for k, v in inspect.signature(AveragedAdam.__init__).parameters.items()}
    assert (defaults["average"], defaults["average_decay"], defaults["average_ramp"], defaults["average_start"]) == ("ema", 0.999, False, 0)
    assert guarded[1:] == ["flat", "lr", "betas", "eps", "weight_decay", "cosine_t_max", "eta_min", "zero_grads", "max_grad_norm",
                           "decoupled", "warmup_steps", "warmup_start"]                  # untouched
    assert list(inspect.signature(FlatAdam.__init__).parameters)[1:] == guarded[1:9]
    flat = _flat()
    opt = AveragedAdam(flat, max_grad_norm=2.5, average="equal", average_start=3, average_ramp=True)
    assert opt.average_mode == "equal" and opt.average_start == 3 and opt.average_ramp and opt.max_grad_norm == 2.5
    assert opt.average.dtype == torch.float32 and torch.equal(opt.average, flat.flat_params)
    assert opt.average.data_ptr() != flat.flat_params.data_ptr()
    assert opt.n_averaged.dtype == torch.int64 and opt.n_averaged.dim() == 0 and int(opt.n_averaged) == 0
    assert opt.swapped is False
    assert AveragedAdam.watch_loss is GuardedAdam.watch_loss and AveragedAdam.health is GuardedAdam.health


@pytest.mark.parametrize("kw,match", [
    (dict(average="median"), "average"),
    (dict(average=None), "average"),
    (dict(average_decay=1.0), "average_decay"),
    (dict(average_decay=-0.1), "average_decay"),
    (dict(average_decay=float("nan")), "average_decay"),
    (dict(average_start=-1), "average_start"),
    (dict(average_start=1.5), "average_start"),
    (dict(max_grad_norm=-1.0), "max_grad_norm"),                      # GuardedAdam's checks still run
])
def test_averaged_adam_refuses_bad_arguments_on_the_host(kw, match):
    from position_induced_transformer_amd.ddp import AveragedAdam
    with pytest.raises(ValueError, match=match):
        AveragedAdam(_flat(), **kw)


TENSORS = {"FlatAdam": {"exp_avg", "exp_avg_sq", "step_count"},
           "GuardedAdam": {"exp_avg", "exp_avg_sq", "step_count", "calls", "state"},
           "AveragedAdam": {"exp_avg", "exp_avg_sq", "step_count", "calls", "state", "average", "n_averaged"}}


def _scramble(opt, seed):
    """Distinct values in every tensor of the state (no step can run on the host)."""
    g = torch.Generator().manual_seed(seed)
    for t in opt._state_tensors().values():
        if t.is_floating_point():
            t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64))
        else:
            t.copy_(torch.randint(1, 1000, t.shape, generator=g))


@pytest.mark.parametrize("name", sorted(TENSORS))
def test_optimizer_state_round_trip(name, tmp_path):
    from position_induced_transformer_amd import ddp
    cls = getattr(ddp, name)
    kw = dict(lr=2e-3, betas=(0.8, 0.95), weight_decay=0.01, cosine_t_max=12, eta_min=1e-5)
    if name != "FlatAdam":
        kw.update(max_grad_norm=0.5, decoupled=True, warmup_steps=2, warmup_start=0.1)
    if name == "AveragedAdam":
        kw.update(average="ema", average_decay=0.9, average_ramp=True, average_start=1)
    opt = cls(_flat(), **kw)
    _scramble(opt, 1)
    state = opt.state_dict()
    tensors = {k for k, v in state.items() if torch.is_tensor(v)}
    assert tensors == TENSORS[name] and set(state) == tensors | {"config"}
    live = opt._state_tensors()
    for k in tensors:                                                 # CPU copies, no aliases
        assert state[k].device.type == "cpu" and state[k].dtype == live[k].dtype and torch.equal(state[k], live[k])
        assert state[k].data_ptr() != live[k].data_ptr()
    config = state["config"]
    assert all(type(v) in (int, float, bool, str) for v in config.values())
    assert config["class"] == name and config["n"] == opt.flat.flat.numel() == 16
    assert (config["lr"], config["beta1"], config["beta2"], config["eps"], config["weight_decay"]) == (2e-3, 0.8, 0.95, 1e-8, 0.01)
    assert (config["cosine_t_max"], config["eta_min"]) == (12, 1e-5)
    if name != "FlatAdam":
        assert (config["max_grad_norm"], config["decoupled"], config["warmup_steps"], config["warmup_start"]) == (0.5, True, 2, 0.1)
    if name == "AveragedAdam":
        assert (config["average"], config["average_decay"], config["average_ramp"], config["average_start"]) == ("ema", 0.9, True, 1)
    path = os.path.join(tmp_path, "opt.pt")
    torch.save(state, path)
    loaded = torch.load(path, weights_only=True)
    other = cls(_flat(), **kw)
    _scramble(other, 2)
    addresses = {k: t.data_ptr() for k, t in other._state_tensors().items()}
    other.load_state_dict(loaded)
    for k, t in other._state_tensors().items():
        assert torch.equal(t, live[k]), k
        assert t.data_ptr() == addresses[k], k                        # copied in place
    assert not other.scalars.any()                                    # not part of the state: the ticket stays 0


def test_load_state_dict_strict_names_what_differs():
    from position_induced_transformer_amd.ddp import AveragedAdam, GuardedAdam
    kw = dict(lr=1e-3, cosine_t_max=12, max_grad_norm=0.5, average_decay=0.9)
    opt = AveragedAdam(_flat(), **kw)
    _scramble(opt, 3)
    state = opt.state_dict()
    for changed, match in ((dict(lr=2e-3), r"\blr\b"), (dict(average_decay=0.99), "average_decay"), (dict(cosine_t_max=13), "cosine_t_max")):
        other = AveragedAdam(_flat(), **{**kw, **changed})
        with pytest.raises(ValueError, match=match):
            other.load_state_dict(state)
        assert not other.exp_avg.any()                                # refused before anything was copied
        other.load_state_dict(state, strict=False)                    # the tensors alone
        for k, t in other._state_tensors().items():
            assert torch.equal(t, state[k]), k
        assert other.lr == changed.get("lr", 1e-3) and other.average_decay == changed.get("average_decay", 0.9)      # settings stay
    # another size: always
    bigger = AveragedAdam(_flat(rows=11), **kw)
    for strict in (True, False):
        with pytest.raises(ValueError, match=r"\bn\b"):
            bigger.load_state_dict(state, strict=strict)
    # a state without its config and with a wrong shape is refused by the shape
    bare = {k: v for k, v in state.items() if k != "config"}
    with pytest.raises(ValueError, match="shape"):
        bigger.load_state_dict(bare, strict=False)
    # a GuardedAdam state lacks the average
    guarded = GuardedAdam(_flat(), lr=1e-3, cosine_t_max=12, max_grad_norm=0.5)
    with pytest.raises(ValueError, match="average"):
        opt.load_state_dict(guarded.state_dict())
    with pytest.raises(ValueError, match="class"):
        guarded.load_state_dict(state)                                # strict: the class is part of the config
    guarded.load_state_dict(state, strict=False)
    assert torch.equal(guarded.exp_avg, opt.exp_avg) and torch.equal(guarded.state, opt.state)


def test_swapped_refuses_step_and_state():
    from position_induced_transformer_amd.ddp import AveragedAdam
    opt = AveragedAdam(_flat())
    state = opt.state_dict()
    opt.swapped = True                                                # (the exchange itself is a launch: tests/test_gpu_run_state.py)
    with pytest.raises(RuntimeError, match="swapped"):
        opt.step()
    with pytest.raises(RuntimeError, match="swapped"):
        opt.state_dict()
    with pytest.raises(RuntimeError, match="swapped"):
        opt.load_state_dict(state)
    with pytest.raises(RuntimeError, match="swapped"):
        with opt.averaged():
            pass
    assert opt.swapped is True
    opt.swapped = False
    opt.load_state_dict(state)


def test_averaged_model_state_replaces_parameters_by_identity():
    from position_induced_transformer_amd.ddp import AveragedAdam, FlatGradients
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))
    model[2].bias.requires_grad_(False)                               # frozen: not in the flat buffers
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = AveragedAdam(flat)
    opt.average.copy_(torch.arange(opt.average.numel(), dtype=torch.float32))
    state = opt.averaged_model_state(model)
    own = model.state_dict()
    assert list(state) == list(own)
    params = dict(model.named_parameters())
    for key, value in state.items():
        if key in params and params[key].requires_grad:
            off = flat.offsets[[id(q) for q in flat.params].index(id(params[key]))]
            assert torch.equal(value.reshape(-1), torch.arange(off, off + value.numel(), dtype=torch.float32)), key
            assert value.shape == own[key].shape and value.data_ptr() != opt.average[off:].data_ptr()
        else:
            assert torch.equal(value, own[key]), key                  # buffers and frozen parameters: the model's
    twin = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))
    twin.load_state_dict(state, strict=True)
    assert torch.equal(twin[0].weight.detach().reshape(-1), torch.arange(12, dtype=torch.float32))


# ----------------------------------------------------------------------------- engine.DeviceFeed
class _Step:
    """What DeviceFeed needs of a step, on the host."""
    graph = None
    _feed = None
    n_valid = None
    len_in = len_out = None

    def __init__(self, batch):
        self.func_in, self.target = torch.zeros(batch, 4, 1), torch.zeros(batch, 4, 1)
        self.mesh_in = self.mesh_out = torch.zeros(4, 2)

    def _check_mesh_update(self, mesh_in, mesh_out):
        pass


def _feed(batch=4, n=24, **kw):
    from position_induced_transformer_amd.engine import DeviceFeed
    data = {"func_in": torch.zeros(n, 4, 1), "target": torch.zeros(n, 4, 1)}
    return DeviceFeed(_Step(batch), data, **{**dict(seed=5, rank=0, world_size=1), **kw})


def test_device_feed_state():
    feed = _feed()
    feed.seek(9)
    state = feed.state_dict()
    assert state == dict(cursor=9, n_samples=24, batch=4, world_size=1, seed=5, shuffle=True, drop_last=True, steps_per_epoch=6)
    assert all(type(v) in (int, bool) for v in state.values())
    twin = _feed()
    assert int(twin.cursor) == 0
    twin.load_state_dict(state)
    assert int(twin.cursor) == 9 and twin.expected_indices(9) == feed.expected_indices(9)
    for kw, match in ((dict(seed=6), "seed"), (dict(batch=3), "batch"), (dict(world_size=2), "world_size"), (dict(n=28), "n_samples"),
                      (dict(shuffle=False), "shuffle")):
        other = _feed(**kw)
        with pytest.raises(ValueError, match=match):
            other.load_state_dict(state)
        assert int(other.cursor) == 0
    with pytest.raises(ValueError, match="cursor|negative"):
        twin.load_state_dict({**state, "cursor": -1})
    assert "order" in type(feed).state_dict.__doc__ and "NOT saved" in type(feed).state_dict.__doc__


def test_train_step_state_on_the_host(tmp_path):
    """TrainStep.state_dict / load_state_dict without a GPU: the model, a fused optimizer and the format marker (the graph path
    is tests/test_gpu_run_state.py)."""
    from position_induced_transformer_amd import pit as P_
    from position_induced_transformer_amd.ddp import AveragedAdam, FlatGradients
    from position_induced_transformer_amd.engine import RolloutStep, TrainStep

    def build(seed):
        torch.manual_seed(seed)
        model = P_.pit_fixed(2, 1, 1, 16, 2, 4, torch.rand(16, 2), 0.1, 0.1)
        mesh, x = torch.rand(36, 2), torch.zeros(8, 36, 1)
        flat = FlatGradients(model.parameters(), flatten_params=True)
        opt = AveragedAdam(flat, lr=1e-3, average_decay=0.9)
        return model, opt, TrainStep(model, (mesh, x, mesh, x.clone()), 1, 2, optimizer=opt, flat=flat)

    model, opt, step = build(0)
    _scramble(opt, 4)
    state = step.state_dict()
    assert set(state) == {"format", "model_state", "optimizer", "feed"} and state["format"] == 1 and state["feed"] is None
    assert list(state["model_state"]) == list(model.state_dict())     # the reference's key names
    assert all(v.device.type == "cpu" for v in state["model_state"].values())
    assert all(v.data_ptr() != w.data_ptr() for v, w in zip(state["model_state"].values(), model.state_dict().values()))
    path = os.path.join(tmp_path, "run.pt")
    torch.save(state, path)
    loaded = torch.load(path, weights_only=True)
    model2, opt2, step2 = build(1)
    addresses = [q.data_ptr() for q in model2.parameters()]
    assert not torch.equal(opt2.flat.flat_params, opt.flat.flat_params)
    step2.load_state_dict(loaded)
    assert torch.equal(opt2.flat.flat_params, opt.flat.flat_params)   # through the views, in place
    assert [q.data_ptr() for q in model2.parameters()] == addresses
    for k, t in opt2._state_tensors().items():
        assert torch.equal(t, opt._state_tensors()[k]), k
    with pytest.raises(ValueError, match="format"):
        step2.load_state_dict({"model_state": loaded["model_state"]})
    with pytest.raises(ValueError, match="optimizer"):
        step2.load_state_dict({**loaded, "optimizer": None})
    bare = TrainStep(model, (step.mesh_in, step.func_in, step.mesh_out, step.target), 1, 2)
    assert bare.state_dict()["optimizer"] is None
    assert RolloutStep.state_dict is TrainStep.state_dict and RolloutStep.load_state_dict is TrainStep.load_state_dict
    assert "build, capture" in TrainStep.load_state_dict.__doc__ and "load_state_dict" in TrainStep.capture.__doc__
