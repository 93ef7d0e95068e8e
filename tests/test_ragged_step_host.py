"""Host side of ragged batches in engine.TrainStep: the two symbols added to ABI 31 (csrc/pit_ragged_step.hip), their argument
checks, the refusals of a step built with lengths and the range check of set_batch - all from CPU tensors, no GPU needed."""
import ctypes
import os
import py_compile
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_STEP = ("pit_rel_lp_loss_ragged_fwd_grad", "pit_rel_max_norm_ragged")


def test_symbols_join_abi_31():
    from position_induced_transformer_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pit_hip.h")).read()
    assert int(re.search(r"#define PIT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 31
    assert re.search(r"#define PIT_HAS_RAGGED_STEP 1", header)
    assert "utils.py:59-98" in header
    assert "pit_ragged_step.hip" in build.SOURCES
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert handle.pit_version() == 31
    for name in RAGGED_STEP:
        assert name in _lib.SIGNATURES and name in _lib.ADDED_LATER and re.search(r"\b%s\(" % name, header), name
        getattr(handle, name)                                        # AttributeError if the library lacks the symbol
    assert len(_lib.SIGNATURES["pit_rel_lp_loss_ragged_fwd_grad"]) == 14 and len(_lib.SIGNATURES["pit_rel_max_norm_ragged"]) == 8


def test_a_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    from position_induced_transformer_amd import _lib

    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name in RAGGED_STEP:
                raise AttributeError(name)
            return getattr(self._real, name)
    real_cdll = ctypes.CDLL
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Stale(real_cdll(path)))
    with pytest.raises(RuntimeError, match="rebuild"):
        _lib.lib()


def test_entries_refuse_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    NULL, SIZE = -1, -2                                              # PIT_ERR_NULL, PIT_ERR_SIZE
    # pit_rel_lp_loss_ragged_fwd_grad(tru, pred, len, batch, npts, nch, p, norms, loss, workspace, d_pred_unit, clear_buf, clear_n, stream)
    good = [p, p, p, 2, 4, 1, 2, p, p, p, p, p, 4, None]
    loss = L.pit_rel_lp_loss_ragged_fwd_grad
    for i, what in ((0, "tru"), (1, "pred"), (2, "len"), (7, "norms"), (8, "loss"), (9, "workspace")):
        args = list(good)
        args[i] = None
        assert loss(*args) == NULL, what
    for i, bad, what in ((3, 0, "batch"), (3, -1, "batch"), (3, 65536, "batch"), (4, 0, "npts"), (5, 0, "nch"), (6, 0, "p"),
                         (12, -1, "clear_n")):
        args = list(good)
        args[i] = bad
        assert loss(*args) == SIZE, (what, bad)
    args = list(good)
    args[11] = None                                                  # clear_n > 0 without a buffer
    assert loss(*args) == SIZE
    # pit_rel_max_norm_ragged(tru, pred, len, batch, npts, nch, out, stream)
    good = [p, p, p, 2, 4, 1, p, None]
    rmax = L.pit_rel_max_norm_ragged
    for i, what in ((0, "tru"), (1, "pred"), (2, "len"), (6, "out")):
        args = list(good)
        args[i] = None
        assert rmax(*args) == NULL, what
    for i, bad, what in ((3, 0, "batch"), (3, 65536, "batch"), (4, 0, "npts"), (5, -3, "nch")):
        args = list(good)
        args[i] = bad
        assert rmax(*args) == SIZE, (what, bad)


def _cpu_step(**kw):
    from position_induced_transformer_amd import engine, tasks
    torch.manual_seed(0)
    model = tasks.pit_elasticity(2, 1, 1, 32, 2, 2, None, 0.05, 0.05)
    mesh, func, target, _ = tasks.ragged_clouds([40, 17, 33], 40, seed=1)
    return engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, **kw), (mesh, func, target)


def test_train_step_refusals_from_cpu_tensors():
    from position_induced_transformer_amd import engine, tasks
    with pytest.raises(ValueError, match="pred_affine"):
        _cpu_step(len_in=[40, 17, 33], pred_affine=(torch.ones(40, 1), torch.zeros(40, 1)))
    darcy = tasks.pit_darcy(2, 1, 1, 32, 2, 2, tasks.grid_mesh_2d(4), 0.5, 0.5)
    mesh = tasks.grid_mesh_2d(6)
    batch = (mesh, torch.randn(2, 6, 6, 1), mesh, torch.randn(2, 6, 6, 1))
    with pytest.raises(ValueError, match="len_in"):
        engine.TrainStep(darcy, batch, 1, 2, len_in=[36, 20])
    with pytest.raises(ValueError, match="len_out"):
        engine.TrainStep(darcy, batch, 1, 2, len_out=[36, 20])
    vort = tasks.pit_vorticity(2, 3, 1, 32, 2, 2, tasks.grid_mesh_2d(4, False), 0.5, 0.5)
    with pytest.raises(ValueError, match="RolloutStep"):
        engine.RolloutStep(vort, (mesh, torch.randn(2, 6, 6, 3), torch.randn(2, 6, 6, 2)), 2, 1, 2, len_in=[36, 20])
    with pytest.raises(ValueError, match="outside"):
        _cpu_step(len_in=[40, 41, 33])
    with pytest.raises(ValueError, match="one entry per sample"):
        _cpu_step(len_in=[40, 17])

    class AnyKeyword(tasks.pit_elasticity):                          # **kw accepts the keywords
        def forward(self, mesh_in, func_in, mesh_out, **kw):
            return super().forward(mesh_in, func_in, mesh_out, **kw)
    model = AnyKeyword(2, 1, 1, 32, 2, 2, None, 0.05, 0.05)
    m, f, t, _ = tasks.ragged_clouds([40, 17], 40, seed=2)
    step = engine.TrainStep(model, (m, f, m, t), 1, 2, len_in=[40, 17])
    assert step.len_in.dtype == torch.int32 and step.len_in.tolist() == [40, 17] and step.len_out is None


def test_lengths_become_static_tensors_and_set_batch_checks_lists():
    step, (mesh, func, target) = _cpu_step(len_in=[40, 17, 33])
    assert step.len_in.dtype == torch.int32 and step.len_in.tolist() == [40, 17, 33] and step.len_out is None
    assert step._len_loss is step.len_in                             # mesh_out is mesh_in: the loss runs over len_in
    static = step.len_in
    step.set_batch(func, target, mesh, len_in=[1, 40, 2])
    assert step.len_in is static and static.tolist() == [1, 40, 2]
    step.set_batch(func, target, len_in=torch.tensor([5, 6, 7]))     # a tensor (int64 here) is copied as it is
    assert static.tolist() == [5, 6, 7]
    for bad in ([0, 40, 2], [1, 41, 2], [1, 40, -3]):
        with pytest.raises(ValueError, match="outside"):
            step.set_batch(func, target, len_in=bad)
    assert static.tolist() == [5, 6, 7]
    with pytest.raises(ValueError, match="one entry per sample"):
        step.set_batch(func, target, len_in=[1, 2])
    with pytest.raises(ValueError, match="without len_out"):
        step.set_batch(func, target, len_out=[1, 40, 2])
    plain, _ = _cpu_step()
    assert plain.len_in is None and plain.len_out is None and plain._len_loss is None
    with pytest.raises(ValueError, match="without len_in"):
        plain.set_batch(func, target, len_in=[1, 40, 2])
    # distinct query points: the loss runs over len_out; len_in alone leaves the dense loss
    from position_induced_transformer_amd import engine
    other = mesh.clone()
    both = engine.TrainStep(step.model, (mesh, func, other, target), 1, 2, len_in=[40, 17, 33], len_out=[40, 20, 30])
    assert both._len_loss is both.len_out and both.len_out.tolist() == [40, 20, 30]
    only_in = engine.TrainStep(step.model, (mesh, func, other, target), 1, 2, len_in=[40, 17, 33])
    assert only_in._len_loss is None


def test_rel_max_norm_takes_lengths_on_device_tensors_only():
    from position_induced_transformer_amd import utils
    t, q = torch.randn(2, 9, 1), torch.randn(2, 9, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        utils.RelMaxNorm(1)(t, q, [9, 4])
    assert torch.isfinite(utils.RelMaxNorm(1)(t, q))                 # without lengths: the host formula as before


def test_the_example_compiles():
    py_compile.compile(os.path.join(ROOT, "examples", "train_clouds_synthetic.py"), doraise=True)
