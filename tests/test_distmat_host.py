"""Host side of the attention on caller-supplied squared distances: the ABI version and exported symbols, the metric helpers
against the oracle's periodic distances bit for bit, and the refusals that happen before the device check (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import pit_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTMAT = ("pit_distmat_select_fwd", "pit_distmat_fwd", "pit_distmat_bwd", "pit_distmat_bwd_workspace")


def test_abi_version_and_symbols():
    from position_induced_transformer_amd import _lib
    header = open(os.path.join(ROOT, "include", "pit_hip.h")).read()
    assert int(re.search(r"#define PIT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 31
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert handle.pit_version() == 31
    for name in DISTMAT:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
        getattr(handle, name)                                        # AttributeError if the library lacks the symbol
    assert "pit_distmat_bwd_workspace" in _lib.LONG_RETURN
    handle.pit_distmat_bwd_workspace.restype = ctypes.c_long
    assert handle.pit_distmat_bwd_workspace(3, 100, 2) == 3 * 100 * 2 * 4
    assert handle.pit_distmat_bwd_workspace(0, 100, 2) == 0


def test_entries_refuse_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    assert L.pit_distmat_select_fwd(None, 4, 0, 1, 4, 4, 0, 1, None, None) == -1            # PIT_ERR_NULL
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert L.pit_distmat_select_fwd(p, 3, 0, 1, 4, 4, 0, 1, p, None) == -2                  # ld_m < n_in: PIT_ERR_SIZE
    assert L.pit_distmat_select_fwd(p, 4, 8, 2, 4, 4, 0, 1, p, None) == -2                  # samples overlap
    assert L.pit_distmat_select_fwd(p, 4, 0, 1, 4, 4, 4, 1, p, None) == -2                  # rank beyond the row
    args = (p, 4, 0, 4, 4, p, 1, 2, 2, 8, p, 1, 1, p, 0.0, 0, p, 2, 8, 0, 0, p, p)
    assert L.pit_distmat_fwd(*args, 1, None) == -4                                           # bf16 mode: PIT_ERR_UNSUPPORTED
    assert L.pit_distmat_fwd(*args[:1], 3, *args[2:], 0, None) == -2                         # ld_m < n_in


def test_periodic_box_is_the_oracles_periodic2d_bit_for_bit():
    from position_induced_transformer_amd import metric
    for mesh_in in (orc.grid_mesh_2d(8, False), orc.grid_mesh_2d(9, True)):
        mesh_out = torch.rand(37, 2, generator=torch.Generator().manual_seed(1))
        l = orc.period_2d(mesh_in)
        sq = metric.sqdist_periodic_box((l, l))
        assert torch.equal(sq(mesh_in, mesh_in), orc.sqdist_periodic2d(mesh_in, mesh_in))
        assert torch.equal(sq(mesh_out, mesh_in), orc.sqdist_periodic2d(mesh_out, mesh_in))
        lf = float(l)                                                # the period as a python float: the same fp32 value
        assert torch.equal(metric.sqdist_periodic_box((lf, lf))(mesh_out, mesh_in), orc.sqdist_periodic2d(mesh_out, mesh_in))


def test_periodic_box_is_the_oracles_periodic1d_bit_for_bit():
    from position_induced_transformer_amd import metric
    mesh_in = orc.line_mesh_1d(33, 0.0, 2.0)
    mesh_out = 2.0 * torch.rand(20, 1, generator=torch.Generator().manual_seed(2))
    sq = metric.sqdist_periodic_box((orc.period_1d(mesh_in),))
    assert torch.equal(sq(mesh_in, mesh_in), orc.sqdist_periodic1d(mesh_in, mesh_in))
    assert torch.equal(sq(mesh_out, mesh_in), orc.sqdist_periodic1d(mesh_out, mesh_in))


def test_metric_helpers_are_differentiable_and_wrap_only_the_periodic_axes():
    from position_induced_transformer_amd import metric
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(6, 3, generator=g).double(), torch.rand(9, 3, generator=g).double()
    assert torch.equal(metric.sqdist_euclid(x, y), orc.sqdist_euclid(x, y))
    assert torch.equal(metric.sqdist_periodic_box((None, None, None))(x, y), orc.sqdist_euclid(x, y))
    sq = metric.sqdist_periodic_box((1.0, None, 0.5))                # channel-like: x and z wrap, y has walls
    d = (x[:, None] - y[None]).abs()
    ref = torch.minimum(d[..., 0], 1.0 - d[..., 0]) ** 2 + d[..., 1] ** 2 + torch.minimum(d[..., 2], 0.5 - d[..., 2]) ** 2
    assert torch.allclose(sq(x, y), ref, rtol=0, atol=1e-15)
    assert sq(x.unsqueeze(0).expand(2, -1, -1), y.unsqueeze(0).expand(2, -1, -1)).shape == (2, 6, 9)
    xg = x.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: sq(t, y), (xg,))
    with pytest.raises(ValueError, match="coordinates"):
        sq(x[:, :2], y[:, :2])


def test_refusals_before_the_device_check():
    """Raised from CPU tensors: the checks run before anything touches the GPU."""
    from position_induced_transformer_amd import metric, ops
    self_layer, cross_layer = metric.posatt_metric(2, 4, 0.5), metric.posatt_cross_metric(2, 4, 0.5)
    assert tuple(self_layer.lmda.shape) == (2, 1, 1) and isinstance(self_layer.lmda, torch.nn.Parameter)
    mesh, x, m = torch.rand(9, 2), torch.rand(2, 9, 4), torch.rand(9, 9)
    with ops.math_mode("bf16"):
        for call in (lambda: self_layer(mesh, x), lambda: cross_layer(mesh, mesh, x), lambda: self_layer.forward_dist(m, x),
                     lambda: ops.DistPlan(m, 0.5), lambda: self_layer.dist2att(m, self_layer.lmda, 0.5)):
            with pytest.raises(NotImplementedError, match="fp32"):
                call()
    with pytest.raises(NotImplementedError, match="lengths"):
        self_layer(mesh, x, lengths=[9, 4])
    with pytest.raises(NotImplementedError, match="lengths"):
        cross_layer(mesh, mesh, x, len_in=[9, 4])
    with pytest.raises(NotImplementedError, match="lengths"):
        self_layer.forward_dist(m, x, lengths=[9, 4])
    for bad in (torch.rand(9), torch.rand(1, 2, 9, 9)):
        with pytest.raises(ValueError, match="m_dist"):
            ops.DistPlan(bad, 0.5)
        with pytest.raises(ValueError, match="m_dist"):
            self_layer.forward_dist(bad, x)
    with pytest.raises(ValueError, match="fp32"):
        ops.DistPlan(m.double(), 0.5)
    with pytest.raises(ValueError, match="locality"):
        ops.DistPlan(m, 1.5)
    with pytest.raises(ValueError, match="columns"):
        cross_layer.forward_dist(torch.rand(5, 8), x)
    with pytest.raises(ValueError, match="samples"):
        cross_layer.forward_dist(torch.rand(3, 5, 9), x)
    with pytest.raises(ValueError, match="square"):
        self_layer.forward_dist(torch.rand(5, 9), x)
    with pytest.raises(RuntimeError, match="HIP device only"):       # everything in order: only now the device check
        ops.DistPlan(m, 0.5)


def test_pit_metric_is_a_pit_with_foreign_attention_layers():
    from position_induced_transformer_amd import metric, pit
    model = metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05, sqdist=metric.sqdist_periodic_box((1.0, None)),
                              learn_latent=True)
    assert isinstance(model, pit.pit) and isinstance(model.mesh_ltt, torch.nn.Parameter)
    layers = [model.down, *model.conv, model.up]
    assert all(isinstance(a, metric.posatt_metric) and not isinstance(a, pit.posatt) for a in layers)
    assert [type(a) for a in layers] == [metric.posatt_cross_metric, metric.posatt_metric, metric.posatt_metric, metric.posatt_cross_metric]
    assert model._heads_of_block(0, 32) == 0 and model._heads_of_block(1, 32) == 0
    dev = torch.device("cpu")
    assert model._fused_plan(model.mesh_ltt, 2, 32, dev) is None and not model._edge_modules(model.up, model.de)
    names = {k for k, _ in model.named_parameters()}
    assert {"down.lmda", "conv.0.lmda", "conv.1.lmda", "up.lmda", "mesh_ltt"} <= names
    assert "pit_metric" not in pit.__all__ and not hasattr(pit, "posatt_metric")
