"""No GPU: the large farthest-point sampler (pit_fps_large, pit_fps_large_workspace) in header, binding and source list, the
refusals of the entry before any launch and their order, the workspace size, and the refusals of
ops.farthest_point_sample_large and of tasks.pit_cloud_fps beyond the single-launch sampler's envelope on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h
MAX_POINTS, MAX_SAMPLES = 4194304, 16384


# ----------------------------------------------------------------------------- header, binding, sources
def test_header_binding_and_sources_agree_on_the_large_entries():
    from position_induced_transformer_amd import _lib, build
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_FPS_LARGE 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    assert int(re.search(r"^#define PIT_FPS_LARGE_MAX_POINTS (\d+)$", text, flags=re.M).group(1)) == _lib.FPS_LARGE_MAX_POINTS == MAX_POINTS
    assert int(re.search(r"^#define PIT_FPS_LARGE_MAX_SAMPLES (\d+)$", text, flags=re.M).group(1)) == _lib.FPS_LARGE_MAX_SAMPLES == MAX_SAMPLES
    assert int(re.search(r"^#define PIT_FPS_MAX_POINTS (\d+)$", text, flags=re.M).group(1)) == _lib.FPS_MAX_POINTS == 16384
    assert int(re.search(r"^#define PIT_FPS_MAX_POINTS_WIDE (\d+)$", text, flags=re.M).group(1)) == _lib.FPS_MAX_POINTS_WIDE == 4096
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in (("pit_fps_large_workspace", 3), ("pit_fps_large", 15)):
        assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]) == count, name
        assert hasattr(_lib.lib(), name)
    assert "pit_fps_large_workspace" in _lib.LONG_RETURN and _lib.lib().pit_fps_large_workspace.restype is ctypes.c_long
    assert "pit_fps_large.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pit_fps_large.hip"))
    assert "pit_fps.hip" in build.SOURCES
    assert _lib.lib().pit_version() == 31


# ----------------------------------------------------------------------------- refusals of the entry before any launch
_buf = (ctypes.c_longlong * 64)()
P = ctypes.addressof(_buf)
BASE = dict(mesh=P, batch=4, n=972, space_dim=2, mesh_bstride=972 * 2, lengths=None, start=None, start_all=0, m=256, idx=P,
            out_mesh=P, out_len=None, slice_points=0, workspace=P, stream=None)
BIG = MAX_POINTS + 1

TABLE = [
    (dict(mesh=None), NULL),
    (dict(idx=None), NULL),
    (dict(out_mesh=None), NULL),
    (dict(workspace=None), NULL),
    (dict(workspace=None, batch=0), NULL),                            # pointers before sizes
    (dict(workspace=None, slice_points=100), NULL),
    (dict(workspace=None, n=BIG, mesh_bstride=BIG * 2), NULL),        # pointers before the envelope
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
    (dict(slice_points=100), SIZE),
    (dict(slice_points=128), SIZE),
    (dict(slice_points=65792), SIZE),                                 # a multiple of 256 beyond 65536
    (dict(slice_points=-256), SIZE),
    (dict(slice_points=257), SIZE),
    (dict(n=BIG, mesh_bstride=BIG * 2), UNSUPPORTED),
    (dict(n=BIG, space_dim=8, mesh_bstride=BIG * 8), UNSUPPORTED),
    (dict(n=1 << 30, space_dim=1, mesh_bstride=1 << 30), UNSUPPORTED),
    (dict(n=20000, m=MAX_SAMPLES + 1, mesh_bstride=40000), UNSUPPORTED),
    (dict(n=BIG, m=MAX_SAMPLES + 1, mesh_bstride=BIG * 2, slice_points=65536), UNSUPPORTED),
    (dict(n=BIG, mesh_bstride=BIG * 2, batch=0), SIZE),               # sizes before the envelope
    (dict(n=BIG, mesh_bstride=BIG * 2, slice_points=100), SIZE),
    (dict(n=BIG, mesh_bstride=BIG * 2 - 1), SIZE),
    (dict(n=20000, m=20001, mesh_bstride=40000), SIZE),               # m > n is a size, whatever the envelope says of m
    (dict(n=BIG, m=MAX_SAMPLES + 1, space_dim=9, mesh_bstride=BIG * 9), SIZE),
]


@pytest.mark.parametrize("changed,code", TABLE, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(TABLE)])
def test_entry_refuses_before_any_launch(changed, code):
    """Host memory stands in for every pointer: a call that got as far as a launch would fail differently (no device here)."""
    from position_induced_transformer_amd import _lib
    args = dict(BASE, **changed)
    assert _lib.lib().pit_fps_large(*args.values()) == code


def test_workspace_size_positive_on_valid_sizes_and_zero_on_refused_ones():
    from position_induced_transformer_amd import _lib
    ws = _lib.lib().pit_fps_large_workspace
    for b, n, sp in ((1, 1, 0), (1, 1, 256), (4, 972, 0), (4, 972, 256), (2, 16385, 0), (1, MAX_POINTS, 0), (1, MAX_POINTS, 256),
                     (65535, 300, 65536), (65535, MAX_POINTS, 0)):
        got = ws(b, n, sp)
        assert got >= 4 * b * n + 16 * b, (b, n, sp, got)            # a distance per point, two candidates per sample at least
    for b, n, sp in ((0, 972, 0), (-1, 972, 0), (65536, 972, 0), (4, 0, 0), (4, -5, 0), (4, BIG, 0), (4, 972, 100), (4, 972, 128),
                     (4, 972, 65792), (4, 972, -256)):
        assert ws(b, n, sp) == 0, (b, n, sp)
    # the library's choice gives a cloud at most 256 slices: never more candidates than 256 slices would need
    for n in (1, 1024, 1025, 16385, 262144, 262145, 1000000, MAX_POINTS):
        assert 4 * n < ws(1, n, 0) <= 4 * n + 2 * 8 * 256, n
    assert ws(1, 1025, 256) == 4 * 1025 + 2 * 8 * 5                   # 5 slices of 256 points


# ----------------------------------------------------------------------------- refusals of the op and the model, CPU tensors
def test_op_passes_its_shape_checks_beyond_the_small_envelope_and_ends_at_the_device_check():
    from position_induced_transformer_amd import ops
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.farthest_point_sample_large(torch.zeros(1, 16385, 3), 10)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.farthest_point_sample_large(torch.zeros(1, 4097, 8), 10, slice_points=512)
    with pytest.raises(ValueError, match="beyond the sampler's 16384"):           # the single-launch sampler refuses as before
        ops.farthest_point_sample(torch.zeros(1, 16385, 3), 10)
    with pytest.raises(ValueError, match="beyond the sampler's 16384"):
        ops.check_fps_shapes(torch.zeros(1, 16385, 3), 10)
    assert ops.fps_max_points(3) == 16384 and ops.fps_max_points(4) == 4096


def test_op_refusals_are_raised_on_cpu_tensors():
    from position_induced_transformer_amd import ops
    fps = ops.farthest_point_sample_large
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
    for bad in (0, -1, 41, 2.5, True, None):
        with pytest.raises(ValueError, match="n_samples"):
            fps(mesh, bad)
    with pytest.raises(ValueError, match="n_samples 16385 is beyond"):
        fps(torch.zeros(1, 16390, 1), 16385)
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
    for bad in (100, 128, 65792, -256, 256.0, True):
        with pytest.raises(ValueError, match="slice_points"):
            fps(mesh, 10, slice_points=bad)
    # everything in order except the device: the last refusal, still before any launch
    with pytest.raises(RuntimeError, match="HIP device only"):
        fps(mesh, 40, [40, 1, 7], torch.tensor([0, 1, 2]), slice_points=256)
    with pytest.raises(RuntimeError, match="HIP device only"):
        fps(mesh[0], 1)


def test_model_beyond_the_small_envelope_reaches_the_device_check():
    from position_induced_transformer_amd import tasks
    model = tasks.pit_cloud_fps(2, 3, 1, 32, 2, 2, 16, 0.1, 0.2)
    mesh, func = torch.rand(2, 16385, 2), torch.rand(2, 16385, 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model(mesh, func, mesh)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model(mesh, func, mesh, len_in=[16385, 9000])
    wide = tasks.pit_cloud_fps(4, 3, 1, 32, 2, 2, 16, 0.1, 0.2)
    mesh4 = torch.rand(2, 4097, 4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        wide(mesh4, func[:, :4097], mesh4)
