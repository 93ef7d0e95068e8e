"""No GPU: ragged batches on the candidate-list layers - the three pit_distlist_*_ragged_* entries in header and binding, their
refusals before any launch, and every refusal of the Python side (ops.ListPlan, metric.forward_list / forward, pit_metric) raised
from CPU tensors, i.e. before the device check."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pit_hip.h")
RAGGED = ("pit_distlist_select_ragged_fwd", "pit_distlist_ragged_fwd", "pit_distlist_ragged_bwd")
NULL, SIZE, UNSUPPORTED = -1, -2, -4


def test_header_defines_the_macros_and_the_binding_exposes_the_four_entries():
    from position_induced_transformer_amd import _lib
    text = open(HEADER).read()
    for macro in ("PIT_HAS_DISTLIST_RAGGED", "PIT_HAS_KNN_RAGGED"):
        assert re.search(r"^#define %s 1$" % macro, text, flags=re.M) and _lib.DEFINES[macro] == 1
    assert _lib.ABI_VERSION == 31 and _lib.lib().pit_version() == 31      # nothing that existed changed
    for name in RAGGED + ("pit_knn_box_ragged",):
        assert name in _lib.PROTOTYPES and name in _lib.ADDED_LATER, name
        assert hasattr(_lib.lib(), name), name
    # the existing parameters plus the lengths; the rank's fraction is per sample (an array), the rank itself comes from locality
    dense, rag = _lib.PROTOTYPES["pit_distlist_fwd"], _lib.PROTOTYPES["pit_distlist_ragged_fwd"]
    assert [n for n in rag.argnames if n not in ("len_out", "len_in")] == dense.argnames
    assert rag.argtypes[rag.argnames.index("rank_w")] is ctypes.c_void_p and dense.argtypes[dense.argnames.index("rank_w")] is ctypes.c_float
    dense, rag = _lib.PROTOTYPES["pit_distlist_bwd"], _lib.PROTOTYPES["pit_distlist_ragged_bwd"]
    assert [n for n in rag.argnames if n not in ("len_out", "len_in")] == dense.argnames
    sel = _lib.PROTOTYPES["pit_distlist_select_ragged_fwd"].argnames
    assert {"len_out", "len_in", "rank_w", "locality"} <= set(sel) and "rank_k" not in sel
    for name in ("pit_distlist_select_fwd", "pit_distlist_fwd", "pit_distlist_bwd"):      # the dense entries are as they were
        assert "len_in" not in _lib.PROTOTYPES[name].argnames


def test_entries_refuse_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    base = dict(idx=p, sqd=p, ld=4, bstride=16, cap=4, mesh_batch=2, n_out=4, n_in=9, locality=0.1, need_kth=1, len_out=p, len_in=p,
                stats=p, rank_w=p, stream=None)
    sel = lambda **kw: L.pit_distlist_select_ragged_fwd(*({**base, **kw}[n] for n in _lib.PROTOTYPES["pit_distlist_select_ragged_fwd"].argnames))
    assert sel(idx=None) == NULL and sel(rank_w=None) == NULL
    assert sel(ld=3) == SIZE and sel(bstride=8) == SIZE                  # ld < cap; samples overlap
    assert sel(locality=1.5) == SIZE and sel(locality=float("nan")) == SIZE
    assert sel(locality=0.5) == SIZE                                     # rank 4 of the PADDED width beyond a list of 4 slots
    assert sel(cap=2049, ld=4096, bstride=4 * 4096, n_in=9000) == UNSUPPORTED
    args = (p, p, 4, 16, 4, 4, 9, p, 2, 2, 2, 18, p, 1, 1, p, p, 0, p, p, p, 2, 8, 0, 0, p, p)
    assert len(args) + 2 == len(_lib.PROTOTYPES["pit_distlist_ragged_fwd"].argnames)
    assert L.pit_distlist_ragged_fwd(*args, 1, None) == UNSUPPORTED      # bf16 mode
    assert L.pit_distlist_ragged_fwd(*args[:2], 3, *args[3:], 0, None) == SIZE                     # ld < cap
    assert L.pit_distlist_ragged_fwd(*args[:3], 0, *args[4:], 0, None) == SIZE                     # shared lists, a batch of 2
    assert L.pit_distlist_ragged_fwd(*args[:16], None, *args[17:], 0, None) == NULL                # no rank_w array


def test_python_refusals_come_before_the_device_check():
    from position_induced_transformer_amd import metric, ops
    self_layer, cross_layer = metric.posatt_metric(2, 4, 0.02), metric.posatt_cross_metric(2, 4, 0.02)
    j = 500                                                              # k = 9: lists of at least 11 slots
    x = torch.rand(2, j, 4)
    idx, sqd = torch.randint(0, j, (2, 30, 16)), torch.rand(2, 30, 16)
    # lists shared by the batch have no per-sample length: a ValueError
    for call in (lambda: cross_layer.forward_list(idx[0], sqd[0], x, len_in=[9, 4]), lambda: cross_layer.forward_list(idx[0], sqd[0], x, lengths=[9, 4]),
                 lambda: ops.ListPlan(idx[0], sqd[0], j, 0.02, len_out=[9, 4])):
        with pytest.raises(ValueError, match="per-sample"):
            call()
    with pytest.raises(ValueError, match="one entry per sample"):
        cross_layer.forward_list(idx, sqd, x, len_in=[9, 4, 4])
    with pytest.raises(ValueError, match="either lengths"):
        cross_layer.forward_list(idx, sqd, x, lengths=[9, 4], len_in=[9, 4])
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.ListPlan(idx, sqd, j, 0.02, len_in=torch.tensor([9.0, 4.0]))
    with pytest.raises(ValueError, match="too narrow"):                  # the width is checked against the PADDED key count
        cross_layer.forward_list(idx[..., :10], sqd[..., :10], x, len_in=[40, 40])
    with ops.math_mode("bf16"):
        for call in (lambda: cross_layer.forward_list(idx, sqd, x, len_in=[9, 4]), lambda: ops.ListPlan(idx, sqd, j, 0.02, len_in=[9, 4]),
                     lambda: self_layer(torch.rand(2, j, 2), x, lengths=[9, 4])):
            with pytest.raises(NotImplementedError, match="fp32"):
                call()
    with pytest.raises(RuntimeError, match="HIP device only"):           # every check passed: the device check is the next one
        cross_layer.forward_list(idx, sqd, x, len_out=[30, 7], len_in=[j, 90])


def test_layers_on_meshes_say_which_lengths_they_take():
    from position_induced_transformer_amd import metric
    clouds, shared, x = torch.rand(2, 40, 2), torch.rand(12, 2), torch.rand(2, 40, 4)
    geodesic = lambda a, b: metric.sqdist_euclid(a, b)                   # a metric of the caller's: no box_periods
    tensor_period = metric.sqdist_periodic_box((torch.tensor(1.0), None))
    unsupported = [dict(), dict(neighbors="auto"), dict(neighbors="auto", builder="torch"), dict(neighbors=8, builder="hip", sqdist=geodesic),
                   dict(neighbors=8, builder="hip", sqdist=tensor_period)]
    for kw in unsupported:
        with pytest.raises(NotImplementedError, match="lengths.*builder='hip'"):
            metric.posatt_metric(2, 4, 0.1, **kw)(clouds, x, lengths=[40, 7])
        with pytest.raises(NotImplementedError, match="lengths.*builder='hip'"):
            metric.posatt_cross_metric(2, 4, 0.1, **kw)(shared, clouds, x, len_in=[40, 7])
    layer = metric.posatt_cross_metric(2, 4, 0.1, metric.sqdist_periodic_box((1.0, None)), "auto", "hip")
    with pytest.raises(NotImplementedError, match="lengths"):            # the dense matrix of the caller's
        layer.forward_dist(torch.rand(12, 40), x, lengths=[40, 7])
    with pytest.raises(ValueError, match="shared by the batch"):         # the rule of ops.check_mixed
        layer(shared, clouds, x, len_out=[12, 12], len_in=[40, 7])
    with pytest.raises(ValueError, match="shared by the batch"):
        layer(clouds, shared, torch.rand(2, 12, 4), len_in=[12, 12])
    with pytest.raises(ValueError, match="one entry per sample"):
        layer(shared, clouds, x, len_in=[40, 7, 7])
    with pytest.raises(RuntimeError, match="HIP device only"):
        layer(shared, clouds, x, len_in=[40, 7])


def test_pit_metric_takes_lengths_past_the_refusals_of_the_euclidean_ragged_path():
    """pit.encoder / decoder would send a shared latent mesh against clouds with lengths through ops.check_mixed, which refuses
    space_dim > 3, non-Euclidean metrics and a mesh that requires grad: the metric model reaches its own device check instead."""
    from position_induced_transformer_amd import metric
    torch.manual_seed(0)
    sdim = 5
    model = metric.pit_metric(sdim, 1, 1, 8, 2, 1, torch.rand(12, sdim), 0.2, 0.2, sqdist=metric.sqdist_periodic_box((1.0,) + (None,) * (sdim - 1)),
                              learn_latent=True, neighbors="auto", builder="hip")
    mesh, func = torch.rand(2, 40, sdim), torch.rand(2, 40, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model(mesh, func, mesh, len_in=[40, 7])
    with pytest.raises(ValueError, match="latent mesh"):
        model.encoder(mesh, torch.rand(2, 40, 6), model.mesh_ltt, len_in=[40, 7], len_ltt=[12, 12])
    dense = metric.pit_metric(2, 1, 1, 8, 2, 1, torch.rand(12, 2), 0.2, 0.2)
    with pytest.raises(NotImplementedError, match="lengths"):
        dense(mesh[..., :2], func, mesh[..., :2], len_in=[40, 7])
    import inspect
    assert {"len_in", "len_out"} <= set(inspect.signature(metric.pit_metric.forward).parameters)      # what engine.TrainStep asks
