"""GPU: geodesic neighbour lists (csrc/pit_geo.hip; ops.geo_knn, metric.knn_graph / knn_lists_geodesic / pit_cloud_geodesic).

pit_geo_knn is compared BIT FOR BIT - keys, lengths, `next` and status - with its host restatement (ops.geo_knn_restated, pinned
to the Bellman-Ford fixpoint by tests/test_geo_host.py): every path length is a chain of rounded fp32 adds in both, and equal
lengths are ordered by vertex index, so there is no tolerance.  A graph built from coordinates is built on the device
(metric.knn_graph) and handed to the restatement as it is, so both search the same edge lengths.  Every test asserts on the
RESTATED result that its shape still covers what it claims (no truncated row where it says so, ties where it says so)."""
import pytest
import torch

from test_geo_host import INF, GeoRow, c_shape, check_against_fixpoint, fixpoint, has_ties, islands, lattice, subset_keys
from test_gpu_mesh_grad import _err
from test_gpu_shared_latent import FWD_TOL

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _same_bits(got, ref, tag=None):
    for name, a, b in zip(("idx", "dist", "next", "status"), got, ref):
        a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, name)


def _cuda(t):
    return None if t is None else t.cuda()


def _both(adj, w, k, sources=None, key_of=None, len_v=None, reach=None):
    """(the kernel's result, the restatement's) on one graph held on the host."""
    from position_induced_transformer_amd import ops
    got = ops.geo_knn(adj.cuda(), w.cuda(), k, _cuda(sources), _cuda(key_of), len_v, reach)
    ref = ops.geo_knn_restated(adj, w, k, sources, key_of, len_v, reach)
    _same_bits(got, ref, (k, reach))
    return got, ref


def _graph(pts, g, lengths=None):
    """metric.knn_graph on the device, copied to the host."""
    from position_induced_transformer_amd import metric
    adj, w = metric.knn_graph(pts.cuda(), g, lengths=lengths)
    assert adj.dtype == torch.int32 and w.dtype == torch.float32 and adj.shape == pts.shape[:-1] + (g + 1,)
    return adj.cpu(), w.cpu()


C200 = {}


def _c200():
    """The C shape of 200 points, its device-built 8-neighbour graph and the fixpoint of that graph, shared by the tests."""
    if not C200:
        pts = c_shape(200, 11)
        adj, w = _graph(pts, 8)
        C200.update(pts=pts, adj=adj, w=w, dist=fixpoint(adj, w))
    return C200["pts"], C200["adj"], C200["w"], C200["dist"]


# --------------------------------------------------------------------------- 1. the tie rule
def test_tie_rule_on_the_unit_lattice():
    adj, w = lattice(12)
    got, ref = _both(adj, w, 13, reach=64)
    assert int(ref.status.sum()) == 0 and all(has_ties(ref))
    check_against_fixpoint(ref, adj, w, 13)


# --------------------------------------------------------------------------- 2. geodesic is not Euclid
def test_c_shape_lists_differ_from_the_box_lists():
    from position_induced_transformer_amd import metric
    pts, adj, w, dist = _c200()
    got, ref = _both(adj, w, 16, reach=128)
    assert int(ref.status.sum()) == 0 and int((ref.idx < 0).sum()) == 0
    check_against_fixpoint(ref, adj, w, 16, dist=dist)
    lists = metric.knn_lists_geodesic(adj.cuda(), w.cuda(), 16, reach=128)
    assert lists.idx.dtype == torch.int64 and torch.equal(lists.idx.cpu(), ref.idx.long())
    assert torch.equal(lists.sqd.cpu(), ref.dist * ref.dist) and not lists.sqd.requires_grad
    assert int(lists.truncated_rows) == 0 and int(lists.short_rows) == 0 and lists.truncated_rows.is_cuda
    assert int(lists.cut_rows) == 200                                  # (locality 1.0: every row of a list that is not the whole row)
    box = metric.knn_lists_box(pts.cuda(), pts.cuda(), 16)
    differ = int((box.idx.cpu() != lists.idx.cpu()).any(-1).sum())
    print("rows whose geodesic list is not the Euclidean one:", differ)
    assert differ >= 1


# --------------------------------------------------------------------------- 3. zero-length edges
def test_zero_length_edges_between_doubled_points():
    pts = c_shape(60, 12).repeat(2, 1)
    adj, w = _graph(pts, 6)
    got, ref = _both(adj, w, 10, reach=64)
    assert int(ref.status.sum()) == 0 and all(has_ties(ref)) and int((ref.idx[:, -1] < 0).sum()) > 0
    check_against_fixpoint(ref, adj, w, 10)


# --------------------------------------------------------------------------- 4. keys as a subset
@pytest.mark.parametrize("form", ["up", "down", "proc16", "proc64"])
def test_keys_as_a_subset(form):
    adj, w = _graph(c_shape(300, 13), 8)
    key_of, picks = subset_keys(300, 64, 14)
    sources, keys, k, reach = {"up": (None, key_of, 8, 256), "down": (picks, None, 16, 128), "proc16": (picks, key_of, 16, 256),
                               "proc64": (picks, key_of, 64, 512)}[form]
    got, ref = _both(adj, w, k, sources=sources, key_of=keys, reach=reach)
    assert int(ref.status.sum()) == 0
    check_against_fixpoint(ref, adj, w, k, sources=sources, key_of=keys)


# --------------------------------------------------------------------------- 5. ragged batches
LENGTHS = (200, 131, 64)


def _ragged_clouds(seed):
    pts = torch.stack([c_shape(200, seed + s) for s in range(3)])
    for s, n in enumerate(LENGTHS):
        pts[s, n:] = NAN
    return pts


@pytest.mark.parametrize("g", [8, 70], ids=["G9", "G71"])
def test_ragged_batch_is_its_trimmed_samples(g):
    from position_induced_transformer_amd import ops
    pts = _ragged_clouds(20)
    lengths = tuple(max(n, g + 1) for n in LENGTHS) if g > 8 else LENGTHS
    for s, n in enumerate(lengths):
        pts[s, :n] = c_shape(200, 20 + s)[:n]
    adj, w = _graph(pts, g, torch.tensor(lengths, dtype=torch.int32).cuda())
    for s, n in enumerate(lengths):                                   # whatever the padded adjacency rows hold is never read
        adj[s, n:] = 7
        w[s, n:] = NAN
    len_d = torch.tensor(lengths, dtype=torch.int32).cuda()
    reach = 128 if g == 8 else 256                                    # (71 edges a vertex: two steps discover more than 128)
    got, ref = _both(adj, w, 16, len_v=len_d, reach=reach)
    assert got.idx.shape == (3, 200, 16) and int(ref.status.sum()) == 0
    for s, n in enumerate(lengths):
        alone = ops.geo_knn(adj[s, :n].contiguous().cuda(), w[s, :n].contiguous().cuda(), 16, reach=reach)
        _same_bits([t[s, :n] for t in got], alone, ("alone", s))
        assert bool((got.idx[s, n:] == -1).all()) and bool((got.dist[s, n:] == 0).all())
        assert bool((got.next[s, n:] == INF).all()) and bool((got.status[s, n:] == 0).all())
    if g == 8:
        check_against_fixpoint(GeoRow(ref, 1), adj[1], w[1], 16, vs=lengths[1])


def test_shared_graph_against_batched_sources():
    _, adj, w, dist = _c200()
    g = torch.Generator().manual_seed(31)
    sources = torch.stack([torch.randperm(200, generator=g)[:40] for _ in range(3)]).to(torch.int32)
    sources[1, 5], sources[2, 0], sources[2, 39] = -1, 200, 2 ** 31 - 1           # padded rows
    got, ref = _both(adj, w, 16, sources=sources, reach=128)
    assert got.idx.shape == (3, 40, 16) and int(ref.status.sum()) == 0
    for s in range(3):
        check_against_fixpoint(GeoRow(ref, s), adj, w, 16, sources=sources[s], dist=dist)


# --------------------------------------------------------------------------- 6. unreachable keys
def test_unreachable_keys_leave_slots_empty():
    adj, w = islands()
    got, ref = _both(adj, w, 50, reach=128)
    assert int(ref.status.sum()) == 0 and bool((ref.next == INF).all())
    assert bool(((ref.idx >= 0).sum(-1) == 40).all()) and bool((ref.idx[:, 40:] == -1).all())
    check_against_fixpoint(ref, adj, w, 50)


# --------------------------------------------------------------------------- 7. truncation
def test_truncation_is_reported_and_what_is_listed_is_exact():
    from position_induced_transformer_amd import metric
    _, adj, w, dist = _c200()
    got, ref = _both(adj, w, 16, reach=24)                            # (status and every row, truncated ones included: bit-equal)
    n_cut = int(ref.status.sum())
    print("truncated rows at reach 24:", n_cut, "of 200")
    assert 40 <= n_cut <= 160
    host = type(ref)(*(t.cpu() for t in got))
    check_against_fixpoint(host, adj, w, 16, dist=dist)                # complete rows exact, truncated rows exact where filled
    lists = metric.knn_lists_geodesic(adj.cuda(), w.cuda(), 16, reach=24)
    assert int(lists.truncated_rows) == n_cut


# --------------------------------------------------------------------------- 8. reproducibility, capture, memory
def test_two_runs_give_the_same_bits():
    from position_induced_transformer_amd import ops
    _, adj, w, _ = _c200()
    adj_d, w_d = adj.cuda(), w.cuda()
    first = ops.geo_knn(adj_d, w_d, 16, reach=128)
    (torch.randn(512, 512, device="cuda") @ torch.randn(512, 512, device="cuda")).sum().item()    # unrelated work in between
    _same_bits(ops.geo_knn(adj_d, w_d, 16, reach=128), first)


def test_a_captured_call_replays_on_new_coordinates_and_lengths():
    from position_induced_transformer_amd import metric, ops
    sets = [(_ragged_clouds(40 + 3 * t), lengths) for t, lengths in enumerate(((200, 131, 64), (90, 200, 150), (64, 64, 199)))]
    pts, len_d = sets[0][0].clone().cuda(), torch.tensor(sets[0][1], dtype=torch.int32).cuda()

    def run():
        adj, w = metric.knn_graph(pts, 8, lengths=len_d)
        return adj, w, ops.geo_knn(adj, w, 16, len_v=len_d, reach=128)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        adj, w, res = run()
    for t in (1, 2, 0):
        cloud, lengths = sets[t]
        for s, n in enumerate(lengths):                               # the clouds of this set, NaN beyond their lengths
            cloud[s, :n] = c_shape(200, 40 + 3 * t + s)[:n]
            cloud[s, n:] = NAN
        pts.copy_(cloud); len_d.copy_(torch.tensor(lengths, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        ref = ops.geo_knn_restated(adj.cpu(), w.cpu(), 16, len_v=list(lengths), reach=128)
        assert int(ref.status.sum()) == 0
        _same_bits(res, ref, t)


def test_a_large_call_allocates_its_outputs_only():
    """V = 32 768, every vertex a source, k = 32: a ring with chords of 1, 7 and 131 steps, random lengths."""
    from position_induced_transformer_amd import ops
    n, k = 32768, 32
    g = torch.Generator().manual_seed(77)
    u = torch.arange(n).view(n, 1)
    adj = ((u + torch.tensor([1, -1, 7, -7, 131, -131])) % n).to(torch.int32)
    w = 0.5 + torch.rand(n, 6, generator=g)
    adj_d, w_d = adj.cuda(), w.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = ops.geo_knn(adj_d, w_d, k)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    out_bytes = sum(t.numel() * t.element_size() for t in got)
    print("geo_knn at 32768 vertices, k 32: peak memory grew by", grew, "bytes; outputs", out_bytes)
    assert out_bytes == n * k * 8 + n * 8 and grew == out_bytes
    rows = torch.arange(0, n, 2731).to(torch.int32)                   # a dozen rows against the restatement
    ref = ops.geo_knn_restated(adj, w, k, sources=rows)
    assert int(ref.status.sum()) == 0
    pick = rows.long().cuda()
    _same_bits([t[pick] for t in got], ref, "large")


# --------------------------------------------------------------------------- 9. the list layers on geodesic lists
def test_layers_on_geodesic_lists_agree_with_the_dense_layer():
    """forward_list on the builder's lists against forward_dist on the FULL squared-geodesic matrix of the host fixpoint: the same
    kept set, each within the project's tolerances of the oracle (tests/test_gpu_distlist.py's yardstick and helpers)."""
    from position_induced_transformer_amd import metric, ops
    from test_gpu_distlist import FILL, _att, _check, _oracle_layer, _run_layer
    _, adj, w, dist = _c200()
    j, b, q, heads, dim = 200, 2, 0.05, 2, 24
    lists = metric.knn_lists_geodesic(adj.cuda(), w.cuda(), 16, locality=q, reach=128)
    assert int(lists.truncated_rows) == 0 and int(lists.short_rows) == 0 and int(lists.cut_rows) == 0
    idx, sqd = lists.idx.cpu(), lists.sqd.cpu()
    full = torch.from_numpy(dist)
    full = torch.where(torch.isfinite(full), full * full, torch.full_like(full, FILL))
    assert torch.equal(torch.gather(full, -1, idx), sqd)
    torch.manual_seed(82)
    mod = metric.posatt_cross_metric(heads, dim, q).cuda()
    with ops.head_scale_route("host"), torch.no_grad():
        dense_att = mod.dist2att(full.cuda(), mod.lmda, q)
    list_att = _att(idx, sqd, j, mod.lmda.detach(), q, heads)
    assert torch.equal(dense_att != 0, list_att != 0)
    g = torch.Generator().manual_seed(83)
    x, dy = torch.randn(b, j, dim, generator=g), torch.randn(b, j, heads * dim, generator=g)
    ref = _oracle_layer(idx, sqd, j, x, dy, mod.lmda, q, False)
    _check(_run_layer(mod, idx, sqd, x, dy), ref, "geodesic lists")
    m1, x1 = full.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    mod.lmda.grad = None
    with ops.head_scale_route("host"):
        out = mod.forward_dist(m1, x1)
        out.backward(dy.cuda())
    _check((out, x1.grad, mod.lmda.grad, torch.gather(m1.grad.cpu(), -1, idx)), ref, "dense geodesic matrix")


# --------------------------------------------------------------------------- 10. the model
def _model(seed=0):
    from position_induced_transformer_amd import metric
    torch.manual_seed(seed)
    return metric.pit_cloud_geodesic(2, 3, 1, 32, 2, 2, 64, 0.1, 0.1).cuda()


def _clouds(lengths, seed):
    """C-shaped clouds of the given lengths padded to 200 points, NaN in every padded point, input and target value."""
    g = torch.Generator().manual_seed(seed)
    mesh = torch.stack([c_shape(200, seed + 1 + s) for s in range(len(lengths))])
    func = torch.cat((mesh, torch.randn(len(lengths), 200, 1, generator=g)), -1)
    target = torch.randn(len(lengths), 200, 1, generator=g)
    for s, n in enumerate(lengths):
        mesh[s, n:] = NAN; func[s, n:] = NAN; target[s, n:] = NAN
    return mesh.cuda(), func.cuda(), target.cuda()


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_model_is_its_layers_on_the_restated_lists(ragged):
    from position_induced_transformer_amd import metric, ops
    lengths = LENGTHS if ragged else (200, 200, 200)
    model = _model()
    mesh, func, _ = _clouds(lengths, 70)
    func.requires_grad_(True)
    len_d = torch.tensor(lengths, dtype=torch.int32).cuda() if ragged else None
    out = model(mesh, func, mesh, len_in=len_d)
    assert out.shape == (3, 200, 1) and bool(torch.isfinite(out).all())
    real = (torch.arange(200).view(1, 200) < torch.tensor(lengths).view(3, 1)).cuda().unsqueeze(-1)
    torch.where(real, out, torch.zeros_like(out)).square().sum().backward()
    assert bool(torch.isfinite(func.grad[real.expand_as(func)]).all())
    assert bool((func.grad[~real.expand_as(func)] == 0).all())
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in model.parameters())
    # the lists against the restatement, on the graph and the latent points the model used
    adj, w = metric.knn_graph(mesh, 8, lengths=len_d)
    latent = model.last_latent
    picks = latent.idx.cpu()
    key_of = torch.full((3, 200), -1, dtype=torch.int32)
    for s in range(3):
        m = int((picks[s] >= 0).sum())
        assert m == min(64, lengths[s]) and len(set(picks[s, :m].tolist())) == m
        key_of[s, picks[s, :m].long()] = torch.arange(m, dtype=torch.int32)
    len_l = None if not ragged else list(lengths)
    k_down, k_up = metric.default_neighbors(0.1, 200), metric.default_neighbors(0.1, 64)
    ref = (ops.geo_knn_restated(adj.cpu(), w.cpu(), k_down, sources=picks, len_v=len_l),
           ops.geo_knn_restated(adj.cpu(), w.cpu(), 64, sources=picks, key_of=key_of, len_v=len_l),
           ops.geo_knn_restated(adj.cpu(), w.cpu(), k_up, key_of=key_of, len_v=len_l))
    for name, lists, r in zip(("down", "processor", "up"), model.last_lists, ref):
        print(name, "truncated", int(lists.truncated_rows), "short", int(lists.short_rows), "cut", int(lists.cut_rows))
        assert int(r.status.sum()) == 0 and int(lists.truncated_rows) == 0, name
        assert torch.equal(lists.idx.cpu(), r.idx.long()) and torch.equal(lists.sqd.cpu(), r.dist * r.dist), name
    # the same layers composed by hand on the restated lists
    with torch.no_grad():
        pred = model(mesh, func, mesh, len_in=len_d)
        assert torch.equal(pred, out)
        dn, pr, up = [(r.idx.long().cuda(), (r.dist * r.dist).cuda()) for r in ref]
        kw = [{}, {}, {}] if not ragged else [dict(len_out=latent.lengths, len_in=len_d), dict(lengths=latent.lengths),
                                              dict(len_out=len_d, len_in=latent.lengths)]
        ltt = model._mlp_gelu(model.en_layer, model.down.forward_list(*dn, func, **kw[0]))
        for a, mlp in zip(model.conv, model.mlp):
            ltt = model._mlp_gelu(mlp, a.forward_list(*pr, ltt, **kw[1]))
        by_hand = model.de(model.up.forward_list(*up, ltt, **kw[2]))
    assert torch.equal(by_hand, pred)


def test_captured_train_step_serves_two_length_sets():
    from position_induced_transformer_amd import engine
    from test_gpu_distlist_ragged import _check_grads, _grads
    first, second = [200, 131, 64], [97, 200, 160]
    model = _model(1)
    mesh, func, target = _clouds(first, 91)
    step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, len_in=first)
    assert step._len_loss is step.len_in
    step.capture(warmup=1)
    twin = _model(1)
    for lengths, seed in ((second, 92), (first, 91)):
        m, f, t = _clouds(lengths, seed)
        step.set_batch(f, t, mesh_in=m, len_in=lengths)
        step.replay()
        torch.cuda.synchronize()
        assert all(int(l.truncated_rows) == 0 for l in model.last_lists)
        eager = engine.TrainStep(twin, (m, f, m, t), 1, 2, len_in=lengths)
        eager.run_eager()
        torch.cuda.synchronize()
        for s, n in enumerate(lengths):
            assert _err(step.out[s, :n], eager.out[s, :n]) <= FWD_TOL, (lengths, s)
        assert bool(torch.isfinite(step.loss)) and abs(float(step.loss) - float(eager.loss)) <= FWD_TOL * abs(float(eager.loss))
        _check_grads(_grads(model), _grads(twin), f"captured {lengths}")
