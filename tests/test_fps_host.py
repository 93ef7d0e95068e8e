"""No GPU: the farthest-point sampling entry (pit_fps) in header, binding and source list, its refusals before any launch, the
refusals of ops.farthest_point_sample and tasks.pit_cloud_fps on CPU tensors, and the numpy restatement of the semantics
(tests/test_gpu_fps.py: fps_reference) on the cases whose answers are known by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_fps import fps_reference

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h


# ----------------------------------------------------------------------------- header, binding, sources
def test_header_binding_and_sources_agree_on_the_fps_entry():
    from position_induced_transformer_amd import _lib, build
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_FPS 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    assert int(re.search(r"^#define PIT_FPS_MAX_POINTS (\d+)$", text, flags=re.M).group(1)) == _lib.FPS_MAX_POINTS == 16384
    assert int(re.search(r"^#define PIT_FPS_MAX_POINTS_WIDE (\d+)$", text, flags=re.M).group(1)) == _lib.FPS_MAX_POINTS_WIDE == 4096
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "pit_fps"
    assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]) == 13
    assert hasattr(_lib.lib(), name)
    assert "pit_fps.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pit_fps.hip"))
    assert _lib.lib().pit_version() == 31


# ----------------------------------------------------------------------------- refusals of the entry before any launch
_buf = (ctypes.c_longlong * 64)()
P = ctypes.addressof(_buf)
BASE = dict(mesh=P, batch=4, n=972, space_dim=2, mesh_bstride=972 * 2, lengths=None, start=None, start_all=0, m=256, idx=P,
            out_mesh=P, out_len=None, stream=None)

TABLE = [
    (dict(mesh=None), NULL),
    (dict(idx=None), NULL),
    (dict(out_mesh=None), NULL),
    (dict(mesh=None, batch=0), NULL),                                 # pointers before sizes
    (dict(batch=0), SIZE),
    (dict(batch=-1), SIZE),
    (dict(batch=65536), SIZE),                                        # the grid limit
    (dict(n=0), SIZE),
    (dict(n=-7), SIZE),
    (dict(m=0), SIZE),
    (dict(m=-1), SIZE),
    (dict(m=973), SIZE),                                              # more latent points than the padded width
    (dict(space_dim=0), SIZE),
    (dict(space_dim=9), SIZE),
    (dict(mesh_bstride=972 * 2 - 1), SIZE),                           # samples would overlap
    (dict(mesh_bstride=0), SIZE),
    (dict(n=16385, mesh_bstride=16385 * 2), UNSUPPORTED),
    (dict(n=16385, space_dim=3, mesh_bstride=16385 * 3), UNSUPPORTED),
    (dict(n=4097, space_dim=4, mesh_bstride=4097 * 4), UNSUPPORTED),
    (dict(n=4097, space_dim=8, mesh_bstride=4097 * 8), UNSUPPORTED),
    (dict(n=1 << 30, space_dim=1, mesh_bstride=1 << 30), UNSUPPORTED),
    (dict(n=16385, m=16385, batch=0, mesh_bstride=16385 * 2), SIZE),  # sizes before the envelope
]


@pytest.mark.parametrize("changed,code", TABLE, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(TABLE)])
def test_entry_refuses_before_any_launch(changed, code):
    """Host memory stands in for every pointer: a call that got as far as a launch would fail differently (no device here)."""
    from position_induced_transformer_amd import _lib
    args = dict(BASE, **changed)
    assert _lib.lib().pit_fps(*args.values()) == code


# ----------------------------------------------------------------------------- refusals of the op and the model, CPU tensors
def test_op_refusals_are_raised_on_cpu_tensors():
    from position_induced_transformer_amd import ops
    fps = ops.farthest_point_sample
    mesh = torch.rand(3, 40, 2)
    with pytest.raises(RuntimeError, match="HIP device only"):
        fps(mesh, 10)
    with pytest.raises(ValueError, match="fp32"):
        fps(mesh.double(), 10)
    with pytest.raises(ValueError, match="fp32"):
        fps(mesh.bfloat16(), 10)
    with pytest.raises(ValueError, match=r"\(b, n, space_dim\)"):
        fps(torch.rand(40), 10)
    with pytest.raises(ValueError, match=r"\(b, n, space_dim\)"):
        fps(torch.rand(2, 3, 40, 2), 10)
    with pytest.raises(ValueError, match="empty"):
        fps(torch.rand(0, 40, 2), 10)
    with pytest.raises(ValueError, match="beyond 8"):
        fps(torch.rand(3, 40, 9), 10)
    with pytest.raises(ValueError, match="beyond the sampler's 16384"):
        fps(torch.zeros(1, 16385, 3), 10)
    with pytest.raises(ValueError, match="beyond the sampler's 4096"):
        fps(torch.zeros(1, 4097, 4), 10)
    for bad in (0, -1, 41, 2.5, True, None):
        with pytest.raises(ValueError, match="n_samples"):
            fps(mesh, bad)
    with pytest.raises(ValueError, match="one entry per sample"):
        fps(mesh, 10, torch.tensor([40, 40], dtype=torch.int32))
    with pytest.raises(ValueError, match="one entry per sample"):
        fps(mesh, 10, [40, 40, 40, 40])
    with pytest.raises(ValueError, match="lengths must be an int32 or int64"):
        fps(mesh, 10, torch.tensor([40.0, 40.0, 40.0]))
    with pytest.raises(ValueError, match="one entry per sample"):
        fps(mesh, 10, None, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="start must be an int32 or int64"):
        fps(mesh, 10, None, torch.tensor([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="start must be an integer"):
        fps(mesh, 10, None, 1.5)
    # everything in order except the device: the last refusal, still before any launch
    with pytest.raises(RuntimeError, match="HIP device only"):
        fps(mesh, 40, [40, 1, 7], torch.tensor([0, 1, 2]))
    with pytest.raises(RuntimeError, match="HIP device only"):
        fps(mesh[0], 1)


def test_model_refusals_on_cpu_tensors():
    from position_induced_transformer_amd import tasks
    with pytest.raises(ValueError, match="n_latent"):
        tasks.pit_cloud_fps(2, 3, 1, 32, 2, 1, 0, 0.1, 0.1)
    model = tasks.pit_cloud_fps(2, 3, 1, 32, 2, 2, 16, 0.1, 0.2)
    assert model.mesh_ltt is None and model.n_latent == 16 and model.last_latent is None
    assert tuple(model.en_layer.mlp1.weight.shape) == (32, 2 * 3)                 # pit_elasticity's encoder MLP width
    mesh, func = torch.rand(2, 30, 2), torch.rand(2, 30, 3)
    with pytest.raises(ValueError, match="per-sample"):
        model(mesh[0], func, mesh[0])
    with pytest.raises(ValueError, match="n_samples"):
        model(mesh[:, :10], func[:, :10], mesh[:, :10])                           # n_latent beyond the width
    with pytest.raises(ValueError, match="len_in"):
        model(mesh, func, mesh.clone(), len_out=[30, 30])
    with pytest.raises(ValueError, match="len_in"):
        model(mesh, func, mesh.clone(), len_in=[30, 30])                          # (another query mesh needs its own lengths)
    with pytest.raises(NotImplementedError, match="requires grad"):
        model(mesh.clone().requires_grad_(True), func, mesh, len_in=[30, 12], len_out=[30, 12])
    with pytest.raises(RuntimeError, match="HIP device only"):
        model(mesh, func, mesh, len_in=[30, 12])
    with pytest.raises(RuntimeError, match="HIP device only"):
        model(mesh, func, mesh)


# ----------------------------------------------------------------------------- the restatement on hand-checked cases
def _grid8():
    ax = np.arange(8, dtype=np.float32) / np.float32(7)
    return np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)


def test_restatement_grid_duplicates_short_cloud_and_nan_padding():
    idx, mesh, picks = fps_reference(_grid8(), 5)
    assert idx.tolist() == [0, 63, 7, 56, 27] and picks == 5 and np.array_equal(mesh, _grid8()[idx])
    rng = np.random.default_rng(0)
    pts = rng.random((6, 3), dtype=np.float32)
    cloud = np.concatenate((pts, np.repeat(pts[:1], 10, 0)))                      # the tail duplicates point 0
    idx, _, _ = fps_reference(cloud, 12)
    assert sorted(idx[:6].tolist()) == [0, 1, 2, 3, 4, 5] and idx[6:].tolist() == [0] * 6
    idx, mesh, picks = fps_reference(rng.random((9, 2), dtype=np.float32), 8, length=4)
    assert picks == 4 and sorted(idx[:4].tolist()) == [0, 1, 2, 3] and idx[4:].tolist() == [-1] * 4 and not mesh[4:].any()
    cloud = np.full((20, 2), np.nan, dtype=np.float32)
    cloud[:7] = rng.random((7, 2), dtype=np.float32)
    idx, mesh, picks = fps_reference(cloud, 10, length=7, start=100)
    assert picks == 7 and idx[0] == 6 and np.isfinite(mesh).all() and idx.max() < 7
    assert mesh.dtype == np.float32 and idx.dtype == np.int32
