"""No GPU: the k-nearest-keys entries (pit_knn_box, pit_knn_rows) in header, binding and source list, their refusals before any
launch and in the header's order, the refusals of ops.knn_box / knn_rows / metric.knn_lists_box and of the new keywords on CPU
tensors, and the numpy restatement (ops.knn_box_restated) on cases whose answers are known by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pit_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h


def header_const(name: str) -> int:
    return int(re.search(r"^#define " + name + r" (\d+)\b", open(HEADER).read(), flags=re.M).group(1))


MAX_K = header_const("PIT_KNN_MAX_K")
REG_MAX = header_const("PIT_KNN_REG_MAX_KEYS")


def brute_force(d: np.ndarray, k: int):
    """The header's loop on one row of fp32 distances, with Python's own (stable) sort of the pairs (d_j, j)."""
    pairs = sorted((float(v), j) for j, v in enumerate(d))
    nxt = pairs[k][0] if k < len(pairs) else float("inf")
    return [j for _, j in pairs[:k]], [v for v, _ in pairs[:k]], nxt


# ----------------------------------------------------------------------------- header, binding, sources
def test_header_binding_and_sources_agree_on_the_knn_entries():
    from position_induced_transformer_amd import _lib, build, ops
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_KNN 1$", text, flags=re.M)
    assert header_const("PIT_ABI_VERSION") == _lib.ABI_VERSION == 31
    assert MAX_K == _lib.KNN_MAX_K == ops.KNN_MAX_K == 2048 == ops.LIST_MAX_CAP
    assert REG_MAX == _lib.KNN_REG_MAX_KEYS == ops.KNN_REG_MAX_KEYS and REG_MAX % 256 == 0
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("pit_knn_box", 14), ("pit_knn_rows", 11), ("pit_knn_last_form", 0)):
        assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[name]) == n_args, name
        assert hasattr(_lib.lib(), name)
    assert "pit_knn.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pit_knn.hip"))
    assert _lib.lib().pit_version() == 31


# ----------------------------------------------------------------------------- refusals of the entries before any launch
_buf = (ctypes.c_longlong * 64)()
P = ctypes.addressof(_buf)
BOX = dict(mesh_out=P, mesh_in=P, batch=3, n_out=900, n_in=5000, space_dim=2, out_stride=900, in_stride=0, periods=None, k=64,
           idx=P, dist=P, next=P, stream=None)
BOX_TABLE = [
    (dict(mesh_out=None), NULL),
    (dict(mesh_in=None), NULL),
    (dict(idx=None), NULL),
    (dict(dist=None), NULL),
    (dict(next=None), NULL),
    (dict(next=None, batch=0), NULL),                                 # pointers before sizes
    (dict(mesh_in=None, k=MAX_K + 1), NULL),                          # ... and before the envelope
    (dict(batch=0), SIZE),
    (dict(n_out=0), SIZE),
    (dict(n_in=0), SIZE),
    (dict(n_in=-5), SIZE),
    (dict(space_dim=0), SIZE),
    (dict(space_dim=9), SIZE),
    (dict(out_stride=899), SIZE),                                     # samples would overlap
    (dict(out_stride=-1), SIZE),
    (dict(in_stride=4999), SIZE),
    (dict(k=0), SIZE),
    (dict(k=-1), SIZE),
    (dict(k=5001), SIZE),                                             # more neighbours than keys
    (dict(n_in=40, k=41), SIZE),
    (dict(batch=1 << 12, n_out=1 << 13, out_stride=1 << 13, k=64), SIZE),      # batch * n_out * k = 2^31
    (dict(k=MAX_K + 1), UNSUPPORTED),
    (dict(k=5000), UNSUPPORTED),
    (dict(k=MAX_K + 1, space_dim=9), SIZE),                           # sizes before the envelope
    (dict(k=MAX_K + 1, batch=0), SIZE),
]
ROWS = dict(m=P, ld_m=5008, m_bstride=900 * 5008, batch=3, n_out=900, n_in=5000, k=64, idx=P, dist=P, next=P, stream=None)
ROWS_TABLE = [
    (dict(m=None), NULL),
    (dict(idx=None), NULL),
    (dict(dist=None), NULL),
    (dict(next=None), NULL),
    (dict(m=None, n_in=0), NULL),                                     # pointers before sizes
    (dict(batch=0), SIZE),
    (dict(n_out=0), SIZE),
    (dict(n_in=0), SIZE),
    (dict(ld_m=4999), SIZE),
    (dict(m_bstride=899 * 5008 + 4999), SIZE),                        # samples would overlap
    (dict(m_bstride=-1), SIZE),
    (dict(k=0), SIZE),
    (dict(k=5001), SIZE),
    (dict(batch=1 << 12, n_out=1 << 13, m_bstride=0, k=64), SIZE),
    (dict(k=MAX_K + 1), UNSUPPORTED),
    (dict(k=MAX_K + 1, ld_m=4999), SIZE),                             # sizes before the envelope
]


@pytest.mark.parametrize("changed,code", BOX_TABLE, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(BOX_TABLE)])
def test_box_entry_refuses_before_any_launch(changed, code):
    """Host memory stands in for every pointer: a call that got as far as a launch would fail differently (no device here)."""
    from position_induced_transformer_amd import _lib
    assert _lib.lib().pit_knn_box(*dict(BOX, **changed).values()) == code


@pytest.mark.parametrize("changed,code", ROWS_TABLE, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(ROWS_TABLE)])
def test_rows_entry_refuses_before_any_launch(changed, code):
    from position_induced_transformer_amd import _lib
    assert _lib.lib().pit_knn_rows(*dict(ROWS, **changed).values()) == code


def test_refused_calls_leave_the_last_form_alone():
    from position_induced_transformer_amd import _lib, ops
    before = ops.knn_last_form()
    assert before in (0, 1, 2)
    assert _lib.lib().pit_knn_box(*dict(BOX, k=0).values()) == SIZE
    assert ops.knn_last_form() == before


# ----------------------------------------------------------------------------- refusals of the ops and the metric layer, CPU tensors
def test_python_refusals_come_before_the_device_check():
    from position_induced_transformer_amd import metric, ops
    mo, mi = torch.rand(30, 2), torch.rand(50, 2)
    bad_box = [
        (dict(mesh_out=mo.double()), "fp32"),
        (dict(mesh_out=torch.rand(30)), "tensor"),
        (dict(mesh_out=torch.rand(0, 2)), "empty"),
        (dict(mesh_in=torch.rand(50, 3)), "coordinates"),
        (dict(mesh_out=torch.rand(30, 9), mesh_in=torch.rand(50, 9)), "beyond 8"),
        (dict(mesh_out=torch.rand(2, 30, 2), mesh_in=torch.rand(3, 50, 2)), "samples"),
        (dict(k=0), "k must be"),
        (dict(k=51), "k must be"),
        (dict(k=2.0), "k must be"),
        (dict(k=True), "k must be"),
        (dict(mesh_in=torch.rand(3000, 2), k=MAX_K + 1), "at most 2048"),
        (dict(periods=(1.0,)), "entries"),
        (dict(periods=1.0), "sequence"),
        (dict(periods=(torch.tensor(1.0), None)), "tensor period"),
        (dict(periods=torch.ones(2)), "sequence"),
        (dict(periods=("1", None)), "float or None"),
        (dict(periods=(float("inf"), None)), "finite"),
    ]
    for changed, match in bad_box:
        args = dict(dict(mesh_out=mo, mesh_in=mi, k=4, periods=None), **changed)
        with pytest.raises(ValueError, match=match):
            ops.knn_box(**args)
        with pytest.raises(ValueError, match=match):
            ops.knn_box_restated(**args)
    for m, k, match in ((torch.rand(5), 1, "tensor"), (torch.rand(5, 7).double(), 1, "fp32"), (torch.rand(5, 0), 1, "empty"),
                        (torch.rand(5, 7), 8, "k must be"), (torch.rand(5, 7), 0, "k must be"),
                        (torch.rand(2, 3000), MAX_K + 1, "at most 2048")):
        with pytest.raises(ValueError, match=match):
            ops.knn_rows(m, k)
    # the checks passed: CPU tensors end at the device error
    for call in (lambda: ops.knn_box(mo, mi, 4), lambda: ops.knn_box(mo, mi, 4, (1.0, None)), lambda: ops.knn_rows(torch.rand(5, 7), 7),
                 lambda: metric.knn_lists_box(mo, mi, 8), lambda: metric.knn_lists(metric.sqdist_euclid, mo, mi, 8, select="hip")):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_metric_refusals_are_value_errors():
    from position_induced_transformer_amd import metric
    mo, mi = torch.rand(30, 2), torch.rand(50, 2)
    assert metric.list_capacity(0.1, 50) == 6
    with pytest.raises(ValueError, match="neighbours"):
        metric.knn_lists_box(mo, mi, 5, locality=0.1)                  # narrower than list_capacity
    with pytest.raises(ValueError, match="neighbours"):
        metric.knn_lists_box(mo, mi, 51)
    with pytest.raises(ValueError, match="at most 2048"):
        metric.knn_lists_box(mo, torch.rand(3000, 2), MAX_K + 1)
    with pytest.raises(ValueError, match="tensor period"):
        metric.knn_lists_box(mo, mi, 8, periods=(torch.tensor(1.0), None))
    with pytest.raises(ValueError, match="fp32"):
        metric.knn_lists_box(mo.double(), mi.double(), 8)
    with pytest.raises(ValueError, match="tensor"):
        metric.knn_lists_box(mo[0], mi, 8)
    with pytest.raises(ValueError, match="select"):
        metric.knn_lists(metric.sqdist_euclid, mo, mi, 8, select="rocm")
    with pytest.raises(ValueError, match="at most 2048"):
        metric.knn_lists(metric.sqdist_euclid, mo, torch.rand(3000, 2), MAX_K + 1, select="hip")
    with pytest.raises(ValueError, match="builder"):
        metric.posatt_cross_metric(2, 4, 0.05, neighbors="auto", builder="cuda")
    with pytest.raises(ValueError, match="builder"):
        metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05, neighbors="auto", builder=None)


def test_defaults_are_the_torch_builder():
    import inspect
    from position_induced_transformer_amd import metric
    assert inspect.signature(metric.knn_lists).parameters["select"].default == "torch"
    for cls in (metric.posatt_metric, metric.posatt_cross_metric, metric.pit_metric):
        assert inspect.signature(cls.__init__).parameters["builder"].default == "torch"
    model = metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05, neighbors="auto")
    assert model.down.builder == model.up.builder == "torch"
    model = metric.pit_metric(2, 1, 1, 32, 2, 2, torch.rand(16, 2), 0.05, 0.05, neighbors="auto", builder="hip")
    assert model.down.builder == model.up.builder == "hip" and all(c.builder == "torch" for c in model.conv)


def test_the_default_knn_lists_is_topk_on_cpu_as_before():
    """select='torch' needs no device and no library call: the lists of the brute-force sort, the dense entries' bits."""
    from position_induced_transformer_amd import metric
    g = torch.Generator().manual_seed(5)
    mo, mi = torch.rand(40, 2, generator=g), torch.rand(3, 60, 2, generator=g)
    sq = metric.sqdist_periodic_box((1.0, None))
    lists = metric.knn_lists(sq, mo, mi, 12, chunk=16, locality=0.1)
    dense = sq(mo, mi)
    assert lists.idx.dtype == torch.int64 and lists.idx.shape == (3, 40, 12)
    assert torch.equal(lists.idx.sort(-1).values, torch.argsort(dense, dim=-1, stable=True)[..., :12].sort(-1).values)
    assert torch.equal(lists.sqd, torch.gather(dense, -1, lists.idx)) and int(lists.cut_rows) == 0


def test_box_periods_mark_the_box_metrics():
    from position_induced_transformer_amd import metric
    assert hasattr(metric.sqdist_euclid, "box_periods") and metric.sqdist_euclid.box_periods is None
    assert metric.sqdist_periodic_box((1.0, None)).box_periods == (1.0, None)
    assert metric.sqdist_periodic_box([2.5, 2.5, 2.5]).box_periods == (2.5, 2.5, 2.5)
    t = torch.tensor(1.0)
    assert metric.sqdist_periodic_box((t, None)).box_periods[0] is t
    assert not hasattr(lambda a, b: a, "box_periods")


def test_the_hip_builder_routes_by_box_periods(monkeypatch):
    """A box metric with float periods goes to knn_lists_box, everything else to knn_lists(select='hip')."""
    from position_induced_transformer_amd import metric
    seen = []
    monkeypatch.setattr(metric, "knn_lists_box", lambda mo, mi, k, periods=None, locality=1.0: seen.append(("box", periods, k, locality)))
    monkeypatch.setattr(metric, "knn_lists", lambda sq, mo, mi, k, locality=1.0, select="torch": seen.append((select, k, locality)))
    mo, mi = torch.rand(30, 2), torch.rand(50, 2)
    other = lambda a, b: metric.sqdist_euclid(a, b)                                                    # noqa: E731
    for sq in (metric.sqdist_euclid, metric.sqdist_periodic_box((1.0, None)), metric.sqdist_periodic_box((torch.tensor(1.0), None)), other):
        metric.posatt_cross_metric(2, 4, 0.1, sq, neighbors=9, builder="hip")._build_lists(mo, mi, 9)
    metric.posatt_cross_metric(2, 4, 0.1, metric.sqdist_euclid, neighbors=9)._build_lists(mo, mi, None)
    assert seen == [("box", None, 9, 0.1), ("box", (1.0, None), 9, 0.1), ("hip", 9, 0.1), ("hip", 9, 0.1), ("torch", None, 0.1)]


# ----------------------------------------------------------------------------- the restatement on hand-checked cases
def _grid_shells(i: int, n: int = 8):
    """Squared torus distances (in grid steps) from point i of the n x n grid to every point, as integers."""
    r, c = divmod(i, n)
    out = []
    for j in range(n * n):
        rr, cc = divmod(j, n)
        dr, dc = min(abs(r - rr), n - abs(r - rr)), min(abs(c - cc), n - abs(c - cc))
        out.append(dr * dr + dc * dc)
    return out


def test_restatement_on_the_tie_shells_of_the_8x8_torus():
    """Every point of the periodic 8 x 8 grid sees shells of 1, 4, 4, 4, 8, ... keys at 0, 1, 2, 4, 5, ... squared steps (1/8 and
    its sums are exact in fp32): the list is the shells in order, each shell in ascending key index, whatever k cuts."""
    from position_induced_transformer_amd import ops
    mesh = orc.grid_mesh_2d(8, False)
    assert mesh.shape == (64, 2)
    for k in (1, 4, 5, 9, 13, 64):
        got = ops.knn_box_restated(mesh, mesh, k, (1.0, 1.0))
        assert got.idx.dtype == torch.int32 and got.dist.dtype == torch.float32 and got.idx.shape == (64, k) and got.next.shape == (64,)
        for i in range(64):
            shells = _grid_shells(i)
            want = sorted(range(64), key=lambda j: (shells[j], j))
            assert got.idx[i].tolist() == want[:k], (k, i)
            assert got.dist[i].tolist() == [shells[j] / 64.0 for j in want[:k]], (k, i)
            assert float(got.next[i]) == (shells[want[k]] / 64.0 if k < 64 else float("inf")), (k, i)
    # the first shells by hand, point 0: itself, then 1, 7 (row neighbours) and 8, 56 (column neighbours) at 1/64
    got = ops.knn_box_restated(mesh, mesh, 5, (1.0, 1.0))
    assert got.idx[0].tolist() == [0, 1, 7, 8, 56] and got.dist[0].tolist() == [0.0] + [1 / 64] * 4 and float(got.next[0]) == 2 / 64
    # without the wrap the corner has two neighbours at one step, and (1, 1) next
    got = ops.knn_box_restated(mesh, mesh, 3, None)
    assert got.idx[0].tolist() == [0, 1, 8] and float(got.next[0]) == 2 / 64


def test_restatement_when_every_point_is_the_same():
    from position_induced_transformer_amd import ops
    mesh_in = torch.full((3, 37, 3), 0.3)
    for k in (1, 5, 37):
        got = ops.knn_box_restated(torch.full((4, 3), 0.3), mesh_in, k)
        assert got.idx.shape == (3, 4, k)
        assert torch.equal(got.idx, torch.arange(k, dtype=torch.int32).expand(3, 4, k))
        assert not got.dist.any()
        assert torch.equal(got.next, torch.full((3, 4), 0.0 if k < 37 else float("inf")))


def test_restatement_on_a_periodic_axis_with_points_outside_the_box():
    """Axis 0 wraps with period 1, axis 1 does not.  x = 0.25; the keys' |dx| are 0.5, 0.75, 1.25 (beyond the period: min(t, p - t)
    = -0.25, squared 0.0625), 0; every number is exact in fp32, so the distances are known by hand."""
    from position_induced_transformer_amd import ops
    x = torch.tensor([[0.25, 0.0]])
    y = torch.tensor([[0.75, 0.0], [1.0, 0.5], [1.5, 0.0], [0.25, 2.0], [-1.0, 0.25]])
    # |dx|: .5, .75, 1.25, 0, 1.25 -> wrapped .5, .25, -.25, 0, -.25; dy: 0, .5, 0, 2 (no wrap), .25
    want = [0.25, 0.0625 + 0.25, 0.0625, 4.0, 0.0625 + 0.0625]
    got = ops.knn_box_restated(x, y, 5, (1.0, None))
    assert got.idx[0].tolist() == [2, 4, 0, 1, 3] and got.dist[0].tolist() == sorted(want) and float(got.next[0]) == float("inf")
    got = ops.knn_box_restated(x, y, 2, (1.0, None))
    assert got.idx[0].tolist() == [2, 4] and float(got.next[0]) == 0.25
    # no wrap at all, and a non-positive period, which means the same
    for per in (None, (None, None), (0.0, -1.0)):
        got = ops.knn_box_restated(x, y, 5, per)
        assert got.idx[0].tolist() == [0, 1, 2, 4, 3], per
        assert got.dist[0].tolist() == [0.25, 0.5625 + 0.25, 1.5625, 1.5625 + 0.0625, 4.0], per


@pytest.mark.parametrize("sdim", [1, 3, 5, 8])
def test_restatement_is_brute_force_in_fp32(sdim):
    """Against a scalar loop in numpy fp32, one operation at a time, and Python's sort of the pairs: random points, duplicated
    points, one wrapped axis with a period smaller than the cloud."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(sdim)
    mo, mi = torch.rand(2, 7, sdim, generator=g), torch.rand(2, 33, sdim, generator=g)
    mi[:, 20:] = mi[:, :13]                                          # duplicated keys
    per = [None] * sdim
    per[sdim // 2] = 0.4
    for periods in (None, tuple(per)):
        for k in (1, 6, 33):
            got = ops.knn_box_restated(mo, mi, k, periods)
            for s in range(2):
                for i in range(7):
                    d = np.zeros(33, np.float32)
                    for j in range(33):
                        acc = None
                        for a in range(sdim):
                            t = np.abs(np.float32(mo[s, i, a]) - np.float32(mi[s, j, a]))
                            if periods is not None and periods[a] is not None:
                                t = min(t, np.float32(periods[a]) - t)
                            q = np.float32(t * t)
                            acc = q if acc is None else np.float32(acc + q)
                        d[j] = acc
                    idx, dist, nxt = brute_force(d, k)
                    assert got.idx[s, i].tolist() == idx and got.dist[s, i].tolist() == dist and float(got.next[s, i]) == nxt
