"""Host side of "per-sample clouds on a mesh shared by the batch": ABI 28 and its symbols, the refusals raised before the device
check (CPU tensors, no GPU needed), and the quantile ranks of the cases tests/test_gpu_shared_latent.py is built on."""
import ctypes
import os
import re

import pytest
import torch

import pit_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDED = ("pit_plan_ragged_strided_fwd", "pit_posatt_ragged_strided_fwd", "pit_posatt_ragged_strided_bwd")


def test_abi_28_and_symbols():
    from position_induced_transformer_amd import _lib
    header = open(os.path.join(ROOT, "include", "pit_hip.h")).read()
    assert int(re.search(r"#define PIT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 28
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in STRIDED:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
        getattr(handle, name)
    # two strides more than the ABI 27 entries, which keep their signatures
    for old in ("pit_plan_ragged_fwd", "pit_posatt_ragged_fwd", "pit_posatt_ragged_bwd"):
        new = old.replace("ragged", "ragged_strided")
        assert len(_lib.SIGNATURES[new]) == len(_lib.SIGNATURES[old]) + 2
    assert (len(_lib.SIGNATURES["pit_plan_ragged_fwd"]), len(_lib.SIGNATURES["pit_posatt_ragged_fwd"]),
            len(_lib.SIGNATURES["pit_posatt_ragged_bwd"])) == (16, 30, 36)


def test_ranks_of_the_gpu_cases_mask():
    """floor(q * (len - 1)) >= 1 for every (sample, locality) of the masked cases: clouds of 150 / 97 / 40 points and shared meshes
    of 64 / 100 points at localities 0.05 and 0.3 (len 40, q 0.05: rank 1)."""
    from position_induced_transformer_amd import ops
    for q in (0.05, 0.3):
        for n in (150, 97, 40, 64, 100, 90, 41, 52, 33, 17, 71):
            k, _ = orc.quantile_rank(q, n)
            assert k == ops.quantile_rank(q, n)[0]
            assert k >= (1 if n >= 40 else 0), (q, n, k)
    assert orc.quantile_rank(0.05, 40)[0] == 1


def test_mixed_pair_refusals_before_the_device_check():
    from position_induced_transformer_amd import ops, pit
    shared, cloud = torch.rand(9, 2), torch.rand(2, 12, 2)
    assert ops.mixed_pair(shared, cloud) == "out" and ops.mixed_pair(cloud, shared) == "in"
    assert ops.mixed_pair(shared, shared) is None and ops.mixed_pair(cloud, cloud) is None
    with pytest.raises(ValueError, match="shared"):                      # a length for the shared side
        ops.MeshPlan("euclid", shared, cloud, 0.5, False, len_out=[9, 9], len_in=[12, 5])
    with pytest.raises(ValueError, match="shared"):
        ops.MeshPlan("euclid", cloud, shared, 0.5, False, len_in=[9, 9])
    with pytest.raises(NotImplementedError, match="shared mesh against per-sample clouds"):
        ops.MeshPlan("euclid", shared.clone().requires_grad_(True), cloud, 0.5, False)
    with pytest.raises(NotImplementedError, match="shared mesh against per-sample clouds"):
        ops.MeshPlan("euclid", cloud.clone().requires_grad_(True), shared, 0.5, False, len_out=[12, 5])
    with pytest.raises(NotImplementedError, match="bf16"):
        with ops.math_mode("bf16"):
            ops.MeshPlan("euclid", shared, cloud, 0.5, False, len_in=[12, 5])
    with pytest.raises(NotImplementedError, match="space_dim > 3"):
        ops.MeshPlan("euclid", torch.rand(9, 4), torch.rand(2, 12, 4), 0.5, False, len_in=[12, 5])
    with pytest.raises(ValueError, match="periodic1d"):
        ops.MeshPlan("periodic1d", shared, cloud, 0.5, False, len_in=[12, 5])
    with pytest.raises(RuntimeError, match="batch-free meshes only"):
        ops.MeshPlan("periodic1d", shared, cloud, 0.5, False)
    with pytest.raises(RuntimeError, match="HIP device"):                # accepted as a pair: the next stop is the device check
        ops.MeshPlan("euclid", shared, cloud, 0.5, False, len_in=[12, 5])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.MeshPlan("euclid", cloud, shared, 0.5, False)
    with pytest.raises(ValueError, match="per-sample"):                  # lengths to posatt.forward with a 2-d mesh: as before
        pit.posatt(1, 4, 0.5)(shared, torch.rand(2, 9, 4), lengths=[9, 4])
    with pytest.raises(ValueError, match="shared"):
        pit.posatt_cross(1, 4, 0.5)(shared, cloud, torch.rand(2, 12, 4), len_out=[9, 9], len_in=[12, 5])


def test_task_class():
    from position_induced_transformer_amd import tasks
    ltt = tasks.grid_mesh_2d(4)
    model = tasks.pit_cloud_latent(2, 3, 1, 32, 2, 2, ltt, 0.05, 0.05)
    assert model.mesh_ltt.shape == (16, 2) and model.en_layer.mlp1.in_features == 2 * 3
    assert type(model.down).__name__ == "posatt_cross" and type(model.conv[0]).__name__ == "posatt"
    with pytest.raises(ValueError, match="mesh_ltt"):
        tasks.pit_cloud_latent(2, 3, 1, 32, 2, 2, None, 0.05, 0.05)
    cloud = torch.rand(2, 12, 2)
    with pytest.raises(NotImplementedError, match="shared mesh against per-sample clouds"):
        model(cloud.clone().requires_grad_(True), torch.rand(2, 12, 3), cloud)
    with pytest.raises(ValueError, match="shared"):
        model.encoder(cloud, torch.rand(2, 12, 3), model.mesh_ltt, len_in=[12, 5], len_ltt=[16, 16])
    assert "pit_cloud_latent" not in tasks.TASKS
