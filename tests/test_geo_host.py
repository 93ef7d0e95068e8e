"""Host: the geodesic list builder (csrc/pit_geo.hip; ops.geo_knn / geo_knn_restated, metric.knn_graph / knn_lists_geodesic,
metric.pit_cloud_geodesic) without a device.

ops.geo_knn_restated - the label-setting search the kernel runs, step by step - is pinned here to an INDEPENDENT definition of
the same numbers: the least fixpoint of D(src) = 0, D(v) = min(D(v), fl32(D(u) + w(u, v))) by Bellman-Ford sweeps in numpy fp32
(``fixpoint``), sorted by (D, v) and cut at k (``lists_of``).  Complete rows must agree bit for bit; truncated rows list exact
lengths.  tests/test_gpu_geo.py then compares the kernel with the restatement on the same shapes, which are built here."""
import ctypes
import math

import numpy as np
import pytest
import torch

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h
INF = float("inf")


# ----------------------------------------------------------------------------- graphs
def lattice(n):
    """The n x n four-neighbour unit lattice: adj (n*n, 4) int32 (-1 beyond the border), w = 1."""
    adj = torch.full((n * n, 4), -1, dtype=torch.int32)
    for r in range(n):
        for c in range(n):
            for t, (dr, dc) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
                if 0 <= r + dr < n and 0 <= c + dc < n:
                    adj[r * n + c, t] = (r + dr) * n + c + dc
    return adj, torch.ones(n * n, 4)


def c_shape(n, seed):
    """n points of a C-shaped annulus: r in [0.8, 1], angle in [0.3, 2 pi - 0.3] - the two tips are close in space and far apart
    along the plate."""
    g = torch.Generator().manual_seed(seed)
    r = 0.8 + 0.2 * torch.rand(n, generator=g)
    a = 0.3 + (2 * math.pi - 0.6) * torch.rand(n, generator=g)
    return torch.stack((r * torch.cos(a), r * torch.sin(a)), -1)


def knn_graph_host(pts, g, lengths=None):
    """metric.knn_graph on the host: the restated box search, w = sqrt(dist)."""
    from position_induced_transformer_amd import ops
    got = ops.knn_box_restated(pts, pts, g + 1, len_out=lengths, len_in=lengths)
    return got.idx, torch.sqrt(got.dist)


def islands():
    """Two islands of 40 vertices (5 x 8 four-neighbour lattices, symmetric edge lengths 1 + j / 16) without an edge between them."""
    adj = torch.full((80, 4), -1, dtype=torch.int32)
    w = torch.zeros(80, 4)
    for base in (0, 40):
        for r in range(5):
            for c in range(8):
                u = base + r * 8 + c
                for t, (dr, dc) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
                    if 0 <= r + dr < 5 and 0 <= c + dc < 8:
                        v = base + (r + dr) * 8 + c + dc
                        adj[u, t], w[u, t] = v, 1.0 + ((u * v + u + v) % 7) / 16.0
    return adj, w


# ----------------------------------------------------------------------------- the independent definition
def fixpoint(adj, w, vs=None):
    """D[s, v]: the least fixpoint from every source s < vs by Bellman-Ford sweeps, numpy fp32 adds; inf = unreachable."""
    adj, w = adj.numpy(), w.numpy().astype(np.float32)
    n_vert, n_edge = adj.shape
    vs = n_vert if vs is None else vs
    dist = np.full((vs, vs), np.inf, np.float32)
    dist[np.arange(vs), np.arange(vs)] = 0.0
    while True:
        before = dist.copy()
        for t in range(n_edge):
            u = np.nonzero((adj[:vs, t] >= 0) & (adj[:vs, t] < vs))[0]
            cand = dist[:, u] + w[u, t][None, :]
            assert cand.dtype == np.float32
            np.minimum.at(dist.T, adj[u, t], cand.T)
        if np.array_equal(before, dist):
            return dist


def lists_of(dist_row, key, k):
    """(keys, lengths, the (k+1)-th length or inf) of one fixpoint row: reachable key vertices by (D, v), cut at k."""
    pairs = sorted((float(d), v) for v, d in enumerate(dist_row) if np.isfinite(d) and (key is None or key[v] >= 0))
    nxt = pairs[k][0] if len(pairs) > k else INF
    return [v if key is None else int(key[v]) for _, v in pairs[:k]], [d for d, _ in pairs[:k]], nxt


def check_against_fixpoint(got, adj, w, k, sources=None, key_of=None, vs=None, dist=None):
    """One sample's restated (or kernel) result against the fixpoint: complete rows bit for bit (``next`` exactly when every
    vertex is a key, as a lower bound otherwise); truncated rows list distinct keys in range at exact, ascending lengths."""
    n_vert = adj.shape[0]
    vs = n_vert if vs is None else vs
    dist = fixpoint(adj, w, vs) if dist is None else dist
    key = None if key_of is None else key_of.numpy()
    n_keys = vs if key is None else int((key[:vs] >= 0).sum())
    src = range(n_vert) if sources is None else sources.tolist()
    for i, s in enumerate(src):
        idx, dd, nx, st = got.idx[i].tolist(), got.dist[i].tolist(), float(got.next[i]), int(got.status[i])
        if not 0 <= s < vs:
            assert idx == [-1] * k and dd == [0.0] * k and nx == INF and st == 0, i
            continue
        keys, lengths, nxt = lists_of(dist[s], key, k)
        if st == 0:
            assert idx == keys + [-1] * (k - len(keys)), i
            assert dd == lengths + [0.0] * (k - len(keys)), i
            assert nx == nxt if key is None else nx <= nxt, i
        else:
            filled = [t for t in range(k) if idx[t] >= 0]
            assert filled == list(range(len(filled))) and len(set(idx[:len(filled)])) == len(filled), i
            inv = {(v if key is None else int(key[v])): v for v in range(vs) if key is None or key[v] >= 0}
            assert len(inv) == n_keys and all(idx[t] in inv for t in filled), i
            assert all(dd[t] == float(dist[s][inv[idx[t]]]) for t in filled), i      # (a settled length is final)
            assert dd[:len(filled)] == sorted(dd[:len(filled)]) and dd[len(filled):] == [0.0] * (k - len(filled)), i


def has_ties(got):
    """Per row: does the list hold two equal lengths among its filled slots."""
    rows = [d[i >= 0].tolist() for i, d in zip(got.idx.reshape(-1, got.idx.shape[-1]), got.dist.reshape(-1, got.idx.shape[-1]))]
    return [len(set(r)) < len(r) for r in rows]


def subset_keys(n, m, seed):
    """m of n vertices labelled 0..m-1 in a random order: (key_of (n,) int32, the labelled vertices in key order)."""
    g = torch.Generator().manual_seed(seed)
    picks = torch.randperm(n, generator=g)[:m].to(torch.int32)
    key_of = torch.full((n,), -1, dtype=torch.int32)
    key_of[picks.long()] = torch.arange(m, dtype=torch.int32)
    return key_of, picks


# ----------------------------------------------------------------------------- the restatement against the fixpoint
def test_restatement_on_the_lattice_tie_shells():
    from position_induced_transformer_amd import ops
    adj, w = lattice(12)
    got = ops.geo_knn_restated(adj, w, 13, reach=64)
    assert int(got.status.sum()) == 0 and all(has_ties(got))
    check_against_fixpoint(got, adj, w, 13)


def test_restatement_on_the_c_shape_and_its_truncation():
    from position_induced_transformer_amd import ops
    pts = c_shape(200, 11)
    adj, w = knn_graph_host(pts, 8)
    dist = fixpoint(adj, w)
    got = ops.geo_knn_restated(adj, w, 16, reach=128)
    assert int(got.status.sum()) == 0 and int((got.idx < 0).sum()) == 0
    check_against_fixpoint(got, adj, w, 16, dist=dist)
    box = ops.knn_box_restated(pts, pts, 16)
    assert not torch.equal(box.idx, got.idx)                           # the geodesic neighbourhood is another one
    cut = ops.geo_knn_restated(adj, w, 16, reach=24)
    n_cut = int(cut.status.sum())
    print("truncated rows at reach 24:", n_cut)
    assert 40 <= n_cut <= 160
    check_against_fixpoint(cut, adj, w, 16, dist=dist)


def test_restatement_on_zero_length_edges():
    from position_induced_transformer_amd import ops
    pts = c_shape(60, 12).repeat(2, 1)                                 # every point twice: vertices i and i + 60 coincide
    adj, w = knn_graph_host(pts, 6)
    got = ops.geo_knn_restated(adj, w, 10, reach=64)
    assert int(got.status.sum()) == 0 and all(has_ties(got)) and int((got.idx[:, -1] < 0).sum()) > 0
    check_against_fixpoint(got, adj, w, 10)


@pytest.mark.parametrize("form", ["up", "down", "proc16", "proc64"])
def test_restatement_with_keys_as_a_subset(form):
    from position_induced_transformer_amd import ops
    adj, w = knn_graph_host(c_shape(300, 13), 8)
    key_of, picks = subset_keys(300, 64, 14)
    sources, keys, k, reach = {"up": (None, key_of, 8, 256), "down": (picks, None, 16, 128), "proc16": (picks, key_of, 16, 256),
                               "proc64": (picks, key_of, 64, 512)}[form]
    got = ops.geo_knn_restated(adj, w, k, sources=sources, key_of=keys, reach=reach)
    assert int(got.status.sum()) == 0
    check_against_fixpoint(got, adj, w, k, sources=sources, key_of=keys)


def test_restatement_on_a_ragged_batch_and_islands():
    from position_induced_transformer_amd import ops
    lengths = (200, 131, 64)
    pts = torch.stack([c_shape(200, 20 + s) for s in range(3)])
    for s, n in enumerate(lengths):
        pts[s, n:] = float("nan")
    adj, w = knn_graph_host(pts, 8, lengths)
    for s, n in enumerate(lengths):
        adj[s, n:] = 7
        w[s, n:] = float("nan")
    got = ops.geo_knn_restated(adj, w, 16, len_v=lengths, reach=128)
    assert got.idx.shape == (3, 200, 16) and int(got.status.sum()) == 0
    for s, n in enumerate(lengths):
        alone = ops.geo_knn_restated(adj[s, :n].contiguous(), w[s, :n].contiguous(), 16, reach=128)
        for a, b in zip(got, alone):
            assert torch.equal(a[s, :n], b)
        assert int((got.idx[s, n:] != -1).sum()) == 0 and float(got.dist[s, n:].abs().sum()) == 0.0
        assert bool((got.next[s, n:] == INF).all()) and int(got.status[s, n:].sum()) == 0
        check_against_fixpoint(GeoRow(got, s), adj[s], w[s], 16, vs=n)
    adj, w = islands()
    got = ops.geo_knn_restated(adj, w, 50, reach=128)
    assert int(got.status.sum()) == 0 and bool((got.next == INF).all())
    assert bool(((got.idx >= 0).sum(-1) == 40).all()) and bool((got.idx[:, 40:] == -1).all())
    check_against_fixpoint(got, adj, w, 50)


class GeoRow:
    """Sample s of a batched GeoResult."""
    def __init__(self, got, s):
        self.idx, self.dist, self.next, self.status = got.idx[s], got.dist[s], got.next[s], got.status[s]


# ----------------------------------------------------------------------------- refusals, CPU tensors
def test_python_refusals_come_before_the_device_check():
    from position_induced_transformer_amd import metric, ops
    adj, w = lattice(6)
    bad = [
        (dict(adj=adj.long()), "int32"),
        (dict(w=w.double()), "float32"),
        (dict(adj=adj[0]), "tensor"),
        (dict(w=w[:, :3]), "one shape"),
        (dict(adj=torch.zeros(0, 4, dtype=torch.int32), w=torch.zeros(0, 4)), "empty"),
        (dict(k=0), "k must be"),
        (dict(k=2.0), "k must be"),
        (dict(k=True), "k must be"),
        (dict(k=1025, reach=4096), "at most 1024"),
        (dict(reach=3), "reach"),
        (dict(reach=4097), "reach"),
        (dict(reach=8.0), "reach"),
        (dict(sources=torch.zeros(5, dtype=torch.int64)), "int32"),
        (dict(sources=torch.zeros(2, 3, 5, dtype=torch.int32)), "sources must be"),
        (dict(key_of=torch.zeros(35, dtype=torch.int32)), "vertices"),
        (dict(key_of=torch.zeros(36)), "int32"),
        (dict(adj=adj.expand(2, 36, 4), w=w.expand(2, 36, 4), sources=torch.zeros(3, 5, dtype=torch.int32)), "samples"),
        (dict(len_v=[36, 36]), "one entry per sample"),
    ]
    for changed, match in bad:
        args = dict(dict(adj=adj, w=w, k=4), **changed)
        for fn in (ops.check_geo_shapes, ops.geo_knn, ops.geo_knn_restated):
            with pytest.raises(ValueError, match=match):
                fn(**args)
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.geo_knn(adj, w, 4, len_v=torch.ones(1))
    assert ops.check_geo_shapes(adj, w, 4)[4:] == (4, 32, False) and ops.geo_default_reach(1024) == 4096
    assert ops.check_geo_shapes(adj, w, 4, len_v=[36])[6] is True
    bad_lists = [
        (dict(k=37), "neighbours"),
        (dict(key_of=torch.arange(36, dtype=torch.int32)), "n_keys"),
        (dict(n_keys=20), "without key_of"),
        (dict(key_of=torch.arange(36, dtype=torch.int32), n_keys=37), "n_keys"),
        (dict(adj=adj[0]), "adj must be"),
        (dict(locality=0.5, k=3), "neighbours"),
    ]
    for changed, match in bad_lists:
        with pytest.raises(ValueError, match=match):
            metric.knn_lists_geodesic(**dict(dict(adj=adj, w=w, k=4), **changed))
    with pytest.raises(NotImplementedError, match="no\\s+gradient"):
        metric.knn_lists_geodesic(adj, w.clone().requires_grad_(True), 4)
    with pytest.raises(ValueError, match="g must be"):
        metric.knn_graph(torch.rand(10, 2), 0)
    # the checks passed: CPU tensors end at the device error
    for call in (lambda: ops.geo_knn(adj, w, 4), lambda: metric.knn_lists_geodesic(adj, w, 4),
                 lambda: metric.knn_graph(torch.rand(10, 2), 3)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_model_refusals_come_before_the_device_check():
    from position_induced_transformer_amd import metric
    for kw, match in ((dict(n_latent=0), "n_latent"), (dict(graph_neighbors=0), "graph_neighbors"),
                      (dict(proc_neighbors=True), "proc_neighbors"), (dict(reach=5000), "reach")):
        with pytest.raises(ValueError, match=match):
            metric.pit_cloud_geodesic(**dict(dict(space_dim=2, in_dim=3, out_dim=1, hid_dim=32, n_head=2, n_blocks=1, n_latent=16,
                                                  en_loc=0.1, de_loc=0.1), **kw))
    model = metric.pit_cloud_geodesic(2, 3, 1, 32, 2, 1, 16, 0.1, 0.1)
    mesh, func = torch.rand(2, 40, 2), torch.rand(2, 40, 3)
    adj = torch.zeros(40, 4, dtype=torch.int32)
    small = mesh[:, :9].contiguous()
    for args, kw, match in (((mesh[0], func, mesh[0]), {}, "per-sample"), ((mesh, func, mesh.clone()), {}, "mesh_out must be mesh_in"),
                            ((mesh, func, mesh[:, :20]), {}, "mesh_out must be mesh_in"),
                            ((mesh, func, mesh), dict(adj=adj), "both adj and adj_w"),
                            ((small, func[:, :9], small), {}, "n_latent")):
        with pytest.raises(ValueError, match=match):
            model(*args, **kw)


# ----------------------------------------------------------------------------- the C entry
P = ctypes.addressof(ctypes.create_string_buffer(64))
GEO = dict(adj=P, w=P, adj_bstride=0, batch=3, n_vert=900, n_edge=8, sources=P, src_bstride=256, n_rows=256, key_of=P, key_bstride=900,
           len_v=P, k=16, reach=128, idx=P, dist=P, next=P, status=P, stream=None)
GEO_TABLE = [
    (dict(adj=None), NULL),
    (dict(w=None), NULL),
    (dict(idx=None), NULL),
    (dict(dist=None), NULL),
    (dict(next=None), NULL),
    (dict(status=None), NULL),
    (dict(adj=None, k=0), NULL),                                      # pointers before sizes
    (dict(batch=0), SIZE),
    (dict(n_vert=0), SIZE),
    (dict(n_edge=0), SIZE),
    (dict(n_rows=0), SIZE),
    (dict(k=0), SIZE),
    (dict(reach=15), SIZE),
    (dict(adj_bstride=900 * 8 - 1), SIZE),
    (dict(adj_bstride=-1), SIZE),
    (dict(src_bstride=255), SIZE),
    (dict(key_bstride=899), SIZE),
    (dict(sources=None, src_bstride=0), SIZE),                        # every vertex a source: n_rows must be n_vert
    (dict(sources=None, n_rows=900), SIZE),                           # ... and the stride 0
    (dict(key_of=None), SIZE),                                        # no map, but a stride
    (dict(n_vert=1 << 20, n_edge=1 << 11, adj_bstride=0, key_bstride=0), SIZE),
    (dict(batch=1 << 12, n_rows=1 << 16, src_bstride=0, k=16), SIZE),
    (dict(k=1025, reach=2048), UNSUPPORTED),
    (dict(reach=4097), UNSUPPORTED),
    (dict(k=1025, reach=2048, batch=0), SIZE),                        # sizes before the envelope
]


@pytest.mark.parametrize("changed,code", GEO_TABLE, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(GEO_TABLE)])
def test_entry_refuses_before_any_launch(changed, code):
    """Host memory stands in for every pointer: a call that got as far as a launch would fail differently (no device here)."""
    from position_induced_transformer_amd import _lib
    assert list(GEO) == _lib.PROTOTYPES["pit_geo_knn"].argnames
    assert _lib.lib().pit_geo_knn(*dict(GEO, **changed).values()) == code


def test_header_constants_are_the_envelope():
    from position_induced_transformer_amd import _lib, ops
    assert _lib.DEFINES["PIT_HAS_GEO"] == 1 and _lib.ABI_VERSION == 31
    assert (ops.GEO_MAX_K, ops.GEO_MAX_REACH) == (_lib.DEFINES["PIT_GEO_MAX_K"], _lib.DEFINES["PIT_GEO_MAX_REACH"]) == (1024, 4096)
    assert [ops.geo_default_reach(k) for k in (1, 2, 16, 64, 512, 513)] == [8, 16, 128, 512, 4096, 4096]
