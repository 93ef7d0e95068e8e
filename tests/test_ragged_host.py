"""Host side of the ragged-batch feature: the ABI version and exported symbols, and the argument validation that happens before
the device check (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("pit_plan_ragged_fwd", "pit_posatt_ragged_fwd", "pit_posatt_ragged_bwd", "pit_rel_lp_loss_ragged_fwd",
          "pit_rel_lp_loss_ragged_bwd", "pit_mlp_bwd_params_ordered", "pit_mlp_bwd_params_ordered_workspace")


def test_abi_version_and_symbols():
    from position_induced_transformer_amd import _lib
    header = open(os.path.join(ROOT, "include", "pit_hip.h")).read()
    assert int(re.search(r"#define PIT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 27
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert handle.pit_version() == _lib.ABI_VERSION
    for name in RAGGED:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
        getattr(handle, name)                                        # AttributeError if the library lacks the symbol


def test_existing_entries_keep_their_signatures():
    from position_induced_transformer_amd import _lib
    assert len(_lib.SIGNATURES["pit_posatt_fwd"]) == 33 and len(_lib.SIGNATURES["pit_posatt_bwd"]) == 40
    assert len(_lib.SIGNATURES["pit_plan_fwd"]) == 18 and len(_lib.SIGNATURES["pit_select_fwd"]) == 12


def test_lengths_conversion():
    from position_induced_transformer_amd import ops
    dev = torch.device("cpu")
    t = ops.as_lengths([3, 5], dev, 2)
    assert t.dtype == torch.int32 and t.tolist() == [3, 5]
    t32 = torch.tensor([4, 1], dtype=torch.int32)
    assert ops.as_lengths(t32, dev, 2).data_ptr() == t32.data_ptr()  # used as it is: in-place updates stay visible
    assert ops.as_lengths(torch.tensor([4, 1]), dev, 2).dtype == torch.int32
    with pytest.raises(ValueError, match="one entry per sample"):
        ops.as_lengths([1, 2, 3], dev, 2)
    with pytest.raises(TypeError):
        ops.as_lengths(torch.tensor([1.0, 2.0]), dev, 2)


def test_refusals_before_the_device_check():
    """Raised from CPU tensors: the checks run before anything touches the GPU."""
    from position_induced_transformer_amd import ops, pit
    m3, m2 = torch.rand(2, 9, 2), torch.rand(9, 2)
    ln = [9, 4]
    with pytest.raises(ValueError, match="periodic1d"):
        ops.MeshPlan("periodic1d", m3, m3, 0.5, True, len_out=ln, len_in=ln)
    with pytest.raises(ValueError, match="per-sample"):
        ops.MeshPlan("euclid", m2, m2, 0.5, True, len_out=ln, len_in=ln)
    with pytest.raises(ValueError, match="both"):
        ops.MeshPlan("euclid", m3, m3, 0.5, True, len_out=ln)
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.MeshPlan("euclid", m3.clone().requires_grad_(True), m3, 0.5, False, len_out=ln, len_in=ln)
    with pytest.raises(NotImplementedError, match="space_dim > 3"):
        ops.MeshPlan("euclid", torch.rand(2, 9, 4), torch.rand(2, 9, 4), 0.5, False, len_out=ln, len_in=ln)
    with pytest.raises(NotImplementedError, match="bf16"):
        with ops.math_mode("bf16"):
            ops.MeshPlan("euclid", m3, m3, 0.5, True, len_out=ln, len_in=ln)
    with pytest.raises(ValueError, match="per-sample"):
        pit.posatt_fixed(1, 4, 0.5)(m2, torch.rand(2, 9, 4), lengths=ln)
    with pytest.raises(ValueError, match="per-sample"):
        pit.posatt_cross_periodic2d(1, 4, 0.5)._cross(m2, m2, torch.rand(2, 9, 4), len_out=ln, len_in=ln)


def test_ragged_clouds_generator():
    from position_induced_transformer_amd import tasks
    mesh, func, target, lens = tasks.ragged_clouds([5, 2], 6, pad_value=float("nan"))
    assert mesh.shape == (2, 6, 2) and lens.dtype == torch.int32 and lens.tolist() == [5, 2]
    assert torch.isfinite(mesh[1, :2]).all() and torch.isnan(mesh[1, 2:]).all() and torch.isnan(target[0, 5:]).all()
    with pytest.raises(ValueError):
        tasks.ragged_clouds([7], 6)
