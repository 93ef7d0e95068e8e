"""No GPU: the evaluation entries (pit_eval_metrics, pit_eval_metrics_workspace) in header and binding, their refusals before
any launch, the host-side checks of engine.EvalStep, and engine.merge_eval_state over two gloo ranks."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE = -1, -2                                                   # PIT_ERR_* of include/pit_hip.h


# ----------------------------------------------------------------------------- header and binding
def test_header_and_binding_agree_on_the_eval_entries():
    from position_induced_transformer_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_EVAL_METRICS 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    assert int(re.search(r"^#define PIT_EVAL_STATE_DOUBLES (\d+)$", text, flags=re.M).group(1)) == _lib.EVAL_STATE_DOUBLES == 8
    assert int(re.search(r"^#define PIT_EVAL_MAX_PARTS (\d+)$", text, flags=re.M).group(1)) == _lib.EVAL_MAX_PARTS
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("pit_eval_metrics_workspace", "pit_eval_metrics"):
        assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib(), name)
    assert "pit_eval_metrics_workspace" in _lib.LONG_RETURN
    assert _lib.lib().pit_version() == 31


def test_workspace_size_names_the_dispatch_instance():
    """Parts per series: doubled while each part keeps 1024 points and fewer than 512 workgroups exist, up to 64."""
    from position_induced_transformer_amd import _lib, ops
    assert ops.EVAL_PARTS[-1] == _lib.EVAL_MAX_PARTS
    cases = [((1, 1, 1), 1), ((1, 2047, 1), 1), ((1, 2048, 1), 2), ((1, 4095, 1), 2), ((1, 4096, 1), 4), ((1, 65535, 1), 32),
             ((1, 65536, 1), 64), ((1, 1 << 22, 1), 64), ((10, 177241, 1), 64), ((16, 177241, 1), 32), ((8, 1849, 1), 1),
             ((512, 4096, 1), 1), ((171, 4096, 3), 1), ((85, 4096, 3), 4), ((128, 2048, 3), 2), ((20, 4096, 1), 4)]
    for (b, n, c), parts in cases:
        assert ops.eval_parts(b, n, c) == parts, (b, n, c)
        assert _lib.lib().pit_eval_metrics_workspace(b, n, c) == 16 + 32 * b * c * parts
    for bad in ((0, 4, 1), (2, 0, 1), (2, 4, 0)):
        assert _lib.lib().pit_eval_metrics_workspace(*bad) == SIZE


# ----------------------------------------------------------------------------- refusals before any launch
_buf = (ctypes.c_double * 64)()
P = ctypes.addressof(_buf)

BASE = dict(tru=P, pred=P, pred_scale=None, pred_shift=None, len=None, n_valid=None, batch=2, npts=5, nch=3, p=2, state=P,
            per_sample=P, ps_stride=2, pred_store=P, store_stride=15, capacity=4, advance=1, workspace=P, stream=None)

TABLE = [
    (dict(tru=None), NULL),
    (dict(pred=None), NULL),
    (dict(state=None), NULL),
    (dict(workspace=None), NULL),
    (dict(pred_scale=P), NULL),                                       # one of scale / shift without the other
    (dict(pred_shift=P), NULL),
    (dict(batch=0), SIZE),
    (dict(batch=-1), SIZE),
    (dict(npts=0), SIZE),
    (dict(nch=0), SIZE),
    (dict(p=0), SIZE),
    (dict(batch=65536), SIZE),                                        # the grid limit
    (dict(capacity=-1), SIZE),
    (dict(capacity=0), SIZE),                                         # optional outputs without rows
    (dict(capacity=0, pred_store=None), SIZE),
    (dict(capacity=0, per_sample=None), SIZE),
    (dict(ps_stride=1), SIZE),
    (dict(store_stride=14), SIZE),
    (dict(advance=4), SIZE),                                          # an unknown flag
]


def test_eval_metrics_refuses_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    fn = _lib.lib().pit_eval_metrics
    assert len(BASE) == len(_lib.SIGNATURES["pit_eval_metrics"])     # the table's argument order is the header's
    for changed, code in TABLE:
        assert set(changed) <= set(BASE)
        assert fn(*{**BASE, **changed}.values()) == code, changed


# ----------------------------------------------------------------------------- engine.EvalStep: checks that precede any launch
def _cpu_model(cls=None):
    from position_induced_transformer_amd import pit as P_
    torch.manual_seed(0)
    return P_.pit_fixed(2, 1, 1, 16, 2, 4, torch.rand(16, 2), 0.1, 0.1)


def _cpu_batch(b=3, n=36):
    x = torch.zeros(b, n, 1)
    return torch.rand(n, 2), x, torch.rand(n, 2), x.clone()


def test_eval_step_constructor_checks():
    from position_induced_transformer_amd.engine import EvalStep, RolloutEvalStep
    model = _cpu_model()
    step = EvalStep(model, _cpu_batch(), 1, 2, capacity=7, store_pred=True)
    assert step.state.shape == (8,) and step.state.dtype == torch.float64
    assert step.per_sample.shape == (7, 2) and step.pred.shape == (7, 36, 1)
    assert step.n_valid.dtype == torch.int32 and int(step.n_valid) == 3
    with pytest.raises(ValueError, match="capacity"):
        EvalStep(model, _cpu_batch(), 1, 2, store_pred=True)
    with pytest.raises(ValueError, match="capacity"):
        EvalStep(model, _cpu_batch(), 1, 2, capacity=-1)
    affine = (torch.ones(36, 1), torch.zeros(36, 1))
    with pytest.raises(ValueError, match="pred_affine with lengths"):
        EvalStep(model, _cpu_batch(), 1, 2, pred_affine=affine, len_in=[36, 36, 36])
    with pytest.raises(ValueError, match="pred_is_true"):
        EvalStep(model, _cpu_batch(), 1, 2, pred_affine=affine, pred_is_true=True)
    with pytest.raises(ValueError, match="does not accept the keyword len_in"):      # pit_fixed.forward has no length keywords
        EvalStep(model, _cpu_batch(), 1, 2, len_in=[36, 36, 36])
    mesh, x, _, _ = _cpu_batch()
    roll = RolloutEvalStep(model, (mesh, x, torch.zeros(3, 36, 4)), 4, 1, 2, capacity=5, store_pred=True)
    assert roll.per_sample.shape == (5, 4, 2) and roll.pred.shape == (5, 4, 36, 1)
    with pytest.raises(ValueError, match="steps"):
        RolloutEvalStep(model, (mesh, x, torch.zeros(3, 36, 4)), 0, 1, 2)


def test_eval_step_set_batch_checks():
    from position_induced_transformer_amd.engine import EvalStep
    step = EvalStep(_cpu_model(), _cpu_batch(), 1, 2)
    x = torch.ones(3, 36, 1)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="n_valid"):
            step.set_batch(x, x, n_valid=bad)
    assert float(step.func_in.sum()) == 0.0                           # refused before anything was copied
    with pytest.raises(ValueError, match="built without len_in"):
        step.set_batch(x, x, len_in=[1, 2, 3])
    with pytest.raises(ValueError, match="batch-free"):
        step.set_batch(x, x, mesh_in=torch.rand(36, 2))
    step.set_batch(x, 2 * x, n_valid=0)
    assert int(step.n_valid) == 0
    step.set_batch(3 * x[:2], 4 * x[:2], n_valid=2)                   # a partly filled batch may bring its own rows only
    assert int(step.n_valid) == 2
    assert torch.equal(step.func_in[:2], 3 * x[:2]) and torch.equal(step.func_in[2:], x[2:])
    assert torch.equal(step.target[:2], 4 * x[:2]) and torch.equal(step.target[2:], 2 * x[2:])
    step.set_batch(x, x)
    assert int(step.n_valid) == 3


def test_ops_eval_metrics_refuses_host_tensors_and_grad():
    from position_induced_transformer_amd import ops
    t = torch.zeros(2, 5, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.eval_metrics(t, t, 1, 2, torch.zeros(8, dtype=torch.float64))


# ----------------------------------------------------------------------------- merge_eval_state over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_state(rank):
    return torch.tensor([1.5 + rank, 0.25 * (rank + 1), 0.7 - 0.3 * rank, 0.1 + 0.4 * rank, 5.0 + 2 * rank, 2.0 + rank, 0.0, 0.0],
                        dtype=torch.float64)


def _worker_merge(rank, world, port, out_dir):
    for pth in (ROOT, HERE):
        sys.path.insert(0, pth)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["PIT_IMPORT_SIDE_EFFECTS"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from position_induced_transformer_amd.engine import merge_eval_state
    mine = _rank_state(rank)
    merged = merge_eval_state(mine)
    assert torch.equal(mine, _rank_state(rank))                       # the argument is left alone
    np.save(os.path.join(out_dir, f"merged_{rank}.npy"), merged.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_merge_eval_state_over_two_gloo_ranks(tmp_path):
    mp.spawn(_worker_merge, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = _rank_state(0), _rank_state(1)
    want = a + b
    want[2], want[3] = max(a[2], b[2]), max(a[3], b[3])               # the worst values take the max
    for rank in (0, 1):
        got = torch.from_numpy(np.load(os.path.join(tmp_path, f"merged_{rank}.npy")))
        assert torch.equal(got, want), (rank, got, want)
    assert want[4] == 12.0                                            # the count adds


def test_merge_eval_state_without_a_process_group_is_a_copy():
    from position_induced_transformer_amd.engine import merge_eval_state
    s = _rank_state(1)
    m = merge_eval_state(s)
    assert torch.equal(m, s) and m.data_ptr() != s.data_ptr()
