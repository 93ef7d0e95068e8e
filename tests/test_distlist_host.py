"""Host side of the attention on candidate lists of caller-supplied squared distances: the symbols added to ABI 31, the list
capacity, the refusals that happen before the device check, and knn_lists against brute force on the CPU (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import pit_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTLIST = ("pit_distlist_select_fwd", "pit_distlist_fwd", "pit_distlist_bwd", "pit_distlist_bwd_workspace")


def test_symbols_join_abi_31():
    from position_induced_transformer_amd import _lib
    header = open(os.path.join(ROOT, "include", "pit_hip.h")).read()
    assert int(re.search(r"#define PIT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 31
    assert re.search(r"#define PIT_HAS_DISTLIST 1", header)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert handle.pit_version() == 31
    for name in DISTLIST:
        assert name in _lib.SIGNATURES and name in _lib.ADDED_LATER and re.search(r"\b%s\(" % name, header), name
        getattr(handle, name)                                        # AttributeError if the library lacks the symbol
    assert "pit_distlist_bwd_workspace" in _lib.LONG_RETURN
    chunk = int(re.search(r"#define PIT_DISTLIST_CHUNK (\d+)", header).group(1))
    assert chunk == _lib.DISTLIST_CHUNK == 512
    handle.pit_distlist_bwd_workspace.restype = ctypes.c_long
    # one partial row of 256-column groups per chunk slot and sample
    assert handle.pit_distlist_bwd_workspace(2, 1100, 8, 16) == 2 * _lib.distlist_chunk_slots(1100, 8) * 256 * 4
    assert handle.pit_distlist_bwd_workspace(1, 33, 128, 300) == (33 * 128 // 256 + 1) * 512 * 4
    assert handle.pit_distlist_bwd_workspace(0, 33, 128, 300) == 0


def test_a_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    from position_induced_transformer_amd import _lib

    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name.startswith("pit_distlist"):
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
    assert L.pit_distlist_select_fwd(None, p, 4, 0, 4, 1, 4, 9, 0, 1, p, None) == -1         # PIT_ERR_NULL
    assert L.pit_distlist_select_fwd(p, p, 3, 0, 4, 1, 4, 9, 0, 1, p, None) == -2            # ld < cap: PIT_ERR_SIZE
    assert L.pit_distlist_select_fwd(p, p, 4, 8, 4, 2, 4, 9, 0, 1, p, None) == -2            # samples overlap
    assert L.pit_distlist_select_fwd(p, p, 4, 0, 4, 1, 4, 9, 4, 1, p, None) == -2            # rank beyond the list
    assert L.pit_distlist_select_fwd(p, p, 4096, 0, 2049, 1, 4, 9000, 0, 1, p, None) == -4   # cap > 2048: PIT_ERR_UNSUPPORTED
    args = (p, p, 4, 0, 4, 4, 9, p, 1, 2, 2, 18, p, 1, 1, p, 0.0, 0, p, 2, 8, 0, 0, p, p)
    assert L.pit_distlist_fwd(*args, 1, None) == -4                                           # bf16 mode: PIT_ERR_UNSUPPORTED
    assert L.pit_distlist_fwd(*args[:2], 3, *args[3:], 0, None) == -2                         # ld < cap
    assert L.pit_distlist_fwd(*args[:22], 1, *args[23:], 0, None) == -2                       # copy_inputs with n_out != n_in


def test_list_capacity():
    from position_induced_transformer_amd import metric, ops
    assert metric.list_capacity(0.02, 1849) == 38
    assert metric.list_capacity(0.02, 256) == 7
    assert metric.list_capacity(0.02, 5000) == 101
    for j in (1, 40, 5000):
        assert metric.list_capacity(1.0, j) == 1
    for q, j in ((0.02, 1849), (0.05, 700), (0.3, 77)):
        assert metric.list_capacity(q, j) == ops.quantile_rank(q, j)[0] + 2
    # the default width: capacity plus room for ties, a multiple of 16, never beyond the row
    assert metric.default_neighbors(0.02, 1849) == 64 and metric.default_neighbors(0.05, 256) == 32
    assert metric.default_neighbors(0.5, 40) == 40


def test_refusals_before_the_device_check():
    """Raised from CPU tensors: the checks run before anything touches the GPU."""
    from position_induced_transformer_amd import metric, ops
    self_layer, cross_layer = metric.posatt_metric(2, 4, 0.02), metric.posatt_cross_metric(2, 4, 0.02)
    j = 500                                                          # k = 9: lists of at least 11 slots
    x = torch.rand(2, j, 4)
    idx, sqd = torch.randint(0, j, (30, 16)), torch.rand(30, 16)
    with ops.math_mode("bf16"):
        for call in (lambda: cross_layer.forward_list(idx, sqd, x), lambda: ops.ListPlan(idx, sqd, j, 0.02)):
            with pytest.raises(NotImplementedError, match="fp32"):
                call()
    with pytest.raises(NotImplementedError, match="lengths"):
        cross_layer.forward_list(idx, sqd, x, lengths=[9, 4])
    with pytest.raises(ValueError, match="too narrow"):
        cross_layer.forward_list(idx[:, :10], sqd[:, :10], x)
    with pytest.raises(ValueError, match="too narrow"):
        ops.ListPlan(idx[:, :10], sqd[:, :10], j, 0.02)
    with pytest.raises(ValueError, match="same shape"):
        cross_layer.forward_list(idx, sqd[:, :15], x)
    with pytest.raises(ValueError, match="same shape"):
        cross_layer.forward_list(idx, sqd.unsqueeze(0).expand(2, -1, -1), x)
    with pytest.raises(ValueError, match="idx must be int32 or int64"):
        cross_layer.forward_list(idx.float(), sqd, x)
    with pytest.raises(ValueError, match="sqd must be fp32"):
        cross_layer.forward_list(idx, sqd.double(), x)
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        cross_layer.forward_list(idx[0], sqd[0], x)
    with pytest.raises(ValueError, match="samples"):
        cross_layer.forward_list(idx.unsqueeze(0).expand(3, -1, -1), sqd.unsqueeze(0).expand(3, -1, -1), x)
    with pytest.raises(ValueError, match="N == J"):
        self_layer.forward_list(idx, sqd, x)
    with pytest.raises(ValueError, match="at most 2048"):
        ops.ListPlan(torch.zeros(2, 2049, dtype=torch.int64), torch.zeros(2, 2049), 5000, 1.0)
    with pytest.raises(ValueError, match="locality"):
        ops.ListPlan(idx, sqd, j, 1.5)
    with pytest.raises(RuntimeError, match="HIP device only"):       # everything in order: only now the device check
        cross_layer.forward_list(idx, sqd, x)
    with pytest.raises(RuntimeError, match="HIP device only"):
        metric.posatt_metric(2, 4, 1.0).forward_list(idx[:1, :1].expand(j, 1), sqd[:1, :1].expand(j, 1), x)
    with pytest.raises(ValueError, match="neighbors"):
        metric.posatt_cross_metric(2, 4, 0.02, neighbors="all")


# --------------------------------------------------------------------------- knn_lists on the CPU
def _meshes(sd, batched, seed):
    g = torch.Generator().manual_seed(seed)
    shape_o, shape_i = ((2, 53, sd), (2, 140, sd)) if batched else ((53, sd), (140, sd))
    return torch.rand(*shape_o, generator=g), torch.rand(*shape_i, generator=g)


def _metrics(sd):
    from position_induced_transformer_amd import metric
    part = tuple(1.0 if a % 2 == 0 else None for a in range(sd))
    return [("euclid", metric.sqdist_euclid), ("part-periodic", metric.sqdist_periodic_box(part)),
            ("periodic", metric.sqdist_periodic_box((1.0,) * sd))]


@pytest.mark.parametrize("batched", [False, True], ids=["batch-free", "batched"])
@pytest.mark.parametrize("sd", [1, 2, 3, 5])
def test_knn_lists_are_brute_force_and_bit_equal_to_the_dense_entries(sd, batched):
    from position_induced_transformer_amd import metric
    mo, mi = _meshes(sd, batched, 10 + sd)
    for name, sq in _metrics(sd):
        dense = sq(mo, mi)
        for k, chunk in ((9, 20), (140, 4096)):
            lists = metric.knn_lists(sq, mo, mi, k, chunk=chunk, locality=0.05)       # rank 6: 8 slots at least
            assert lists.idx.shape == dense.shape[:-1] + (k,) and lists.idx.dtype == torch.int64
            brute = torch.argsort(dense, dim=-1, stable=True)[..., :k]
            assert torch.equal(lists.idx.sort(-1).values, brute.sort(-1).values), (name, k)
            assert torch.equal(lists.sqd, torch.gather(dense, -1, lists.idx)), (name, k)
            assert lists.cut_rows.dim() == 0 and int(lists.cut_rows) == 0, (name, k)


def test_knn_lists_count_the_rows_cut_inside_a_tie_shell():
    from position_induced_transformer_amd import metric
    mesh = orc.grid_mesh_2d(8, False)
    sq = metric.sqdist_periodic_box((1.0, 1.0))
    # q = 0.04 over 64 keys: rank 2, so m_(3) lies in the first shell (4 keys at one spacing, ranks 1..4)
    assert metric.list_capacity(0.04, 64) == 4
    cut = metric.knn_lists(sq, mesh, mesh, 4, locality=0.04)         # slots 0..3 hold the point and 3 of its 4 neighbours
    assert int(cut.cut_rows) == 64
    whole = metric.knn_lists(sq, mesh, mesh, 5, locality=0.04)       # the whole shell is listed
    assert int(whole.cut_rows) == 0
    assert int(metric.knn_lists(sq, mesh, mesh, 9, locality=1.0).cut_rows) == 64      # no mask: the dense layer keeps every key
    assert int(metric.knn_lists(sq, mesh, mesh, 64, locality=1.0).cut_rows) == 0
    with pytest.raises(ValueError, match="neighbours"):
        metric.knn_lists(sq, mesh, mesh, 3, locality=0.04)


@pytest.mark.parametrize("batched", [False, True], ids=["batch-free", "batched"])
def test_knn_lists_carry_mesh_gradients_of_the_listed_pairs(batched):
    from position_induced_transformer_amd import metric
    mo, mi = _meshes(2, batched, 31)
    sq = metric.sqdist_periodic_box((1.0, None))
    g = torch.Generator().manual_seed(32)
    mo1, mi1 = mo.double().requires_grad_(True), mi.double().requires_grad_(True)
    lists = metric.knn_lists(sq, mo1, mi1, 12)
    assert lists.sqd.requires_grad and not lists.idx.requires_grad
    w = torch.rand(*lists.sqd.shape, generator=g).double()
    (lists.sqd * w).sum().backward()
    mo2, mi2 = mo.double().requires_grad_(True), mi.double().requires_grad_(True)
    dense_w = torch.zeros(*sq(mo2, mi2).shape, dtype=torch.float64).scatter_(-1, lists.idx, w)
    (sq(mo2, mi2) * dense_w).sum().backward()
    assert torch.allclose(mo1.grad, mo2.grad, rtol=1e-12, atol=1e-14) and torch.allclose(mi1.grad, mi2.grad, rtol=1e-12, atol=1e-14)


def test_pit_metric_takes_neighbors():
    from position_induced_transformer_amd import metric
    model = metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05, neighbors="auto")
    assert model.down.neighbors == "auto" and model.up.neighbors == "auto" and all(c.neighbors is None for c in model.conv)
    assert metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05).down.neighbors is None
    assert metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05, neighbors=24).up.neighbors == 24
