"""GPU: the k nearest keys of every row (csrc/pit_knn.hip; ops.knn_box / knn_rows, metric.knn_lists_box, builder="hip").

pit_knn_box is compared BIT FOR BIT - keys, distances and `next` - with its host restatement (ops.knn_box_restated, pinned to
brute force by tests/test_knn_host.py): the kernel rounds every operation as numpy fp32 does and orders equal distances by key
index, so there is no tolerance.  pit_knn_rows is compared with a stable CPU sort of the same matrix.  The agreement with the
torch builder runs on a 1/1024 lattice, where every fp32 operation of up to 8 coordinates is exact, so the two builders see the
same distances and can differ only in which keys of a tie shell that straddles the cut they take."""
import pytest
import torch

import golden_io as gio
import pit_oracle as orc
from test_gpu_mesh_grad import FUSED, LaunchLog, _err
from test_knn_host import MAX_K, REG_MAX

pytestmark = pytest.mark.gpu

R = REG_MAX
PERIODS = {                                                          # the clouds below span [-0.5, 1.5) on every axis
    "none": lambda s: None,
    "all": lambda s: (1.0,) * s,                                     # points outside the box on every axis
    "mixed": lambda s: tuple(0.75 if a % 2 == 0 else None for a in range(s)),
    "small": lambda s: (0.3,) + (None,) * (s - 1),                   # a period far smaller than the cloud's extent
}
# (space_dim, periods, strides (out, in: s = shared, p = per sample; flat = batch-free), batch, n_out, J, k, points)
CASES = [
    (1, "none", "flat", 1, 1, 1, 1, "random"),
    (2, "none", "flat", 1, 5, 2, 1, "random"),
    (2, "all", "flat", 1, 5, 2, 2, "random"),
    (3, "none", "flat", 1, 67, 63, 33, "random"),
    (3, "mixed", "flat", 1, 5, 63, 62, "random"),
    (1, "all", "flat", 1, 67, 64, 64, "random"),
    (4, "none", "flat", 1, 5, 64, 63, "twice"),
    (5, "mixed", "flat", 1, 67, 65, 2, "random"),
    (6, "none", "flat", 1, 5, 65, 65, "twice"),
    (7, "small", "flat", 1, 1, 65, 64, "random"),
    (8, "none", "flat", 1, 67, R, 33, "random"),
    (2, "all", "flat", 1, 5, R, R, "random"),
    (3, "none", "flat", 1, 5, R, R - 1, "twice"),
    (2, "none", "flat", 1, 67, R + 1, 33, "random"),
    (2, "mixed", "flat", 1, 5, R + 1, R + 1, "random"),
    (1, "none", "flat", 1, 5, R + 1, R, "twice"),
    (3, "small", "flat", 1, 1, R + 1, 1, "random"),
    (2, "none", "flat", 1, 5, 2 * R + 37, min(2 * R + 37, MAX_K), "random"),
    (8, "all", "flat", 1, 5, 2 * R + 37, 2, "random"),
    (4, "mixed", "flat", 1, 67, 2 * R + 37, 33, "twice"),
    (2, "mixed", "ss", 3, 5, 65, 33, "random"),
    (2, "mixed", "sp", 3, 5, 65, 33, "random"),
    (2, "mixed", "ps", 3, 5, 65, 33, "random"),
    (2, "mixed", "pp", 3, 5, 65, 33, "random"),
    (3, "none", "ss", 3, 5, R + 1, 33, "random"),
    (3, "none", "sp", 3, 5, R + 1, 33, "twice"),
    (3, "none", "ps", 3, 5, R + 1, 33, "random"),
    (3, "none", "pp", 3, 5, R + 1, 33, "twice"),
    (6, "all", "pp", 3, 67, 64, 2, "twice"),
    (7, "none", "sp", 3, 1, R, 33, "random"),
    (1, "small", "flat", 1, 67, 2 * R + 37, min(2 * R + 37, MAX_K), "twice"),
    (2, "none", "flat", 1, 67, 700, 48, "random"),
    (3, "mixed", "flat", 1, 5, 1, 1, "random"),
    (5, "all", "flat", 1, 5, 2, 2, "twice"),
    (8, "small", "flat", 1, 5, 63, 1, "random"),
    (4, "none", "ps", 3, 5, 2 * R + 37, min(2 * R + 37, MAX_K), "random"),
    (6, "small", "flat", 1, 5, R + 1, 2, "random"),
    (7, "mixed", "flat", 1, 5, 64, 33, "twice"),
    (1, "none", "flat", 1, 67, 65, 64, "twice"),
    (5, "none", "flat", 1, 5, R + 1, 33, "same"),                    # one tie shell of J keys: the search runs over the index
    (2, "all", "flat", 1, 5, 2 * R + 37, min(2 * R + 37, MAX_K), "same"),
    (3, "none", "pp", 3, 5, 64, 33, "same"),
]


def _cloud(seed, batch, n, sdim, points, per_sample):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand((batch if per_sample else 1), n, sdim, generator=g) * 2.0 - 0.5
    if points == "twice" and n > 1:
        t[:, n - n // 2:] = t[:, :n // 2]                            # every point of the first half comes twice
    if points == "same":
        t[:] = 0.375
    return t


def _case_meshes(i, case):
    sdim, _, strides, batch, n_out, j, _, points = case
    out_ps, in_ps = (False, False) if strides == "flat" else (strides[0] == "p", strides[1] == "p")
    mo = _cloud(1000 + i, batch, n_out, sdim, "same" if points == "same" else "random", out_ps)
    mi = _cloud(2000 + i, batch, j, sdim, points, in_ps)
    if strides == "flat":
        return mo[0], mi[0]
    # a shared mesh of a batched call: batch-free beside a per-sample mesh; two expanded views (sample stride 0) when both are shared
    if strides == "ss":
        return mo.expand(batch, -1, -1), mi.expand(batch, -1, -1)
    return (mo if out_ps else mo[0]), (mi if in_ps else mi[0])


def _dev(t):
    """To the device with the sample stride kept: an expanded view stays one."""
    if t.dim() == 3 and t.shape[0] > 1 and t.stride(0) == 0:
        return t[0].cuda().expand(t.shape[0], -1, -1)
    return t.cuda()


def _same_bits(got, ref, what):
    assert got.idx.dtype == torch.int32 and got.dist.dtype == torch.float32 and got.next.dtype == torch.float32
    assert got.idx.shape == ref.idx.shape and got.next.shape == ref.next.shape, what
    assert torch.equal(got.idx.cpu(), ref.idx), what
    assert torch.equal(got.dist.cpu().view(torch.int32), ref.dist.view(torch.int32)), what
    assert torch.equal(got.next.cpu().view(torch.int32), ref.next.view(torch.int32)), what


# --------------------------------------------------------------------------- 1. pit_knn_box against the restatement, bit for bit
@pytest.mark.parametrize("i", range(len(CASES)), ids=["-".join(str(v) for v in c) for c in CASES])
def test_box_is_the_restatement_bit_for_bit(i):
    from position_induced_transformer_amd import ops
    case = CASES[i]
    sdim, per, strides, batch, n_out, j, k, _ = case
    mo, mi = _case_meshes(i, case)
    periods = PERIODS[per](sdim)
    ref = ops.knn_box_restated(mo, mi, k, periods)
    mo_d, mi_d = _dev(mo), _dev(mi)
    assert mo_d.stride() == mo.stride() and mi_d.stride() == mi.stride()
    got = ops.knn_box(mo_d, mi_d, k, periods)
    assert ops.knn_last_form() == (1 if j <= REG_MAX else 2)
    expect = (n_out, k) if strides == "flat" else (batch, n_out, k)
    assert tuple(got.idx.shape) == expect
    _same_bits(got, ref, case)
    # whatever was compared: in range and distinct
    srt = got.idx.sort(-1).values
    assert int(srt.min()) >= 0 and int(srt.max()) < j and bool((srt[..., 1:] > srt[..., :-1]).all())


def test_the_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == set(range(1, 9)) and {c[1] for c in CASES} == set(PERIODS)
    assert {c[2] for c in CASES if c[3] == 3} == {"ss", "sp", "ps", "pp"}
    assert {c[5] for c in CASES} >= {1, 2, 63, 64, 65, R, R + 1, 2 * R + 37}
    assert {c[4] for c in CASES} == {1, 5, 67}
    ks = {(c[6], c[5]) for c in CASES}
    assert {k for k, _ in ks} >= {1, 2, 33} and any(k == j - 1 for k, j in ks) and any(k == j for k, j in ks)
    assert any(k == MAX_K < j for k, j in ks)
    for strides in ("ss", "sp", "ps", "pp"):                         # the views are what they are called
        case = next(c for c in CASES if c[2] == strides)
        mo, mi = _case_meshes(CASES.index(case), case)
        assert (mo.dim() == 3 and mo.stride(0) != 0) == (strides[0] == "p") and (mi.dim() == 3 and mi.stride(0) != 0) == (strides[1] == "p")


# --------------------------------------------------------------------------- 2. pit_knn_rows against a stable CPU sort
@pytest.mark.parametrize("batch,n_out,j,k", [(2, 67, 65, 33), (1, 5, 64, 64), (2, 5, R + 1, 33), (1, 3, 2 * R + 37, MAX_K), (3, 1, R, R)])
def test_rows_are_a_stable_sort_cut_at_k(batch, n_out, j, k):
    """The matrix is a view into NaN: guard rows above and below every sample, guard columns left and right (ld > J, a base that is
    4-byte aligned only).  The entry is called on buffers of the test's own, between sentinels."""
    from position_induced_transformer_amd import _lib, ops
    g = torch.Generator().manual_seed(j + k)
    ld = j + 5
    buf = torch.full((batch, n_out + 2, ld), float("nan"))
    m = torch.randint(0, 40, (batch, n_out, j), generator=g).float() / 8.0          # many equal entries
    m[..., ::7] = -0.0 * m[..., ::7]                                               # -0.0 counts as 0
    m[:, :, j // 2] = 0.0
    buf[:, 1:n_out + 1, 3:3 + j] = m
    dev = buf.cuda()
    view = dev[:, 1:n_out + 1, 3:3 + j]
    vals, order = torch.sort(m, dim=-1, stable=True)
    want_next = vals[..., k] if k < j else torch.full((batch, n_out), float("inf"))
    # through ops: the view is read in place
    got = ops.knn_rows(view, k)
    assert ops.knn_last_form() == (1 if j <= REG_MAX else 2)
    assert torch.equal(got.idx.cpu().long(), order[..., :k])
    assert torch.equal(got.dist.cpu(), vals[..., :k]) and not torch.signbit(got.dist).any()       # (equal as numbers; zeros come out +0.0)
    assert torch.equal(got.next.cpu(), want_next)
    # the entry on the test's buffers
    pad, rows = 64, batch * n_out
    idx = torch.full((rows * k + 2 * pad,), -77, dtype=torch.int32).cuda()
    dist = torch.full((rows * k + 2 * pad,), -5.0).cuda()
    nxt = torch.full((rows + 2 * pad,), -5.0).cuda()
    rc = _lib.lib().pit_knn_rows(view.data_ptr(), ld, (n_out + 2) * ld, batch, n_out, j, k, idx.data_ptr() + 4 * pad,
                                 dist.data_ptr() + 4 * pad, nxt.data_ptr() + 4 * pad, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for t, fill in ((idx, -77), (dist, -5.0), (nxt, -5.0)):
        assert bool((t[:pad] == fill).all()) and bool((t[-pad:] == fill).all())
    assert torch.equal(idx[pad:-pad].cpu().view(batch, n_out, k), got.idx.cpu())
    assert torch.equal(dist[pad:-pad].cpu().view(batch, n_out, k), got.dist.cpu())
    assert torch.equal(nxt[pad:-pad].cpu().view(batch, n_out), got.next.cpu())


def test_rows_of_anything_give_distinct_keys_in_range():
    """The precondition broken on purpose: NaN, inf and negative entries.  Nothing is promised about the order; every index lies
    in [0, J) and no index comes twice."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(3)
    for j, k in ((65, 33), (R + 1, 200)):
        m = torch.randn(7, j, generator=g)
        m[:, ::5] = float("nan")
        m[:, 1::9] = float("inf")
        m[:, 2::11] = -float("inf")
        srt = ops.knn_rows(m.cuda(), k).idx.sort(-1).values
        assert int(srt.min()) >= 0 and int(srt.max()) < j and bool((srt[:, 1:] > srt[:, :-1]).all())


# --------------------------------------------------------------------------- 3. tie counts
def test_cut_rows_on_the_8x8_torus_are_the_torch_path_s():
    """The counts tests/test_distlist_host.py asserts for knn_lists on the same grid, localities and widths."""
    from position_induced_transformer_amd import metric
    mesh = orc.grid_mesh_2d(8, False).cuda()
    per = (1.0, 1.0)
    for k, locality, want in ((4, 0.04, 64), (5, 0.04, 0), (9, 1.0, 64), (64, 1.0, 0)):
        lists = metric.knn_lists_box(mesh, mesh, k, periods=per, locality=locality)
        assert lists.cut_rows.dim() == 0 and lists.cut_rows.is_cuda and int(lists.cut_rows) == want, (k, locality)
        rows = metric.knn_lists(metric.sqdist_periodic_box(per), mesh, mesh, k, locality=locality, select="hip")
        assert int(rows.cut_rows) == want, (k, locality)
        assert torch.equal(rows.idx, lists.idx) and torch.equal(rows.sqd, lists.sqd)        # 1/8 steps: both see exact distances
    with pytest.raises(ValueError, match="neighbours"):
        metric.knn_lists_box(mesh, mesh, 3, periods=per, locality=0.04)


# --------------------------------------------------------------------------- 4. agreement with the torch builder
AGREE = [(300, 1000, 64, (None, None)), (257, 4097, 128, (1.0, None, 0.5)), (100, 5000, MAX_K, (1.0, 1.0)), (64, 65, 64, (None,)),
         (50, 700, 48, (None,) * 8)]


@pytest.mark.parametrize("n,j,k,per", AGREE, ids=[f"{n}x{j}-k{k}-{len(p)}d" for n, j, k, p in AGREE])
def test_lists_agree_with_the_torch_builder_on_a_lattice(n, j, k, per):
    from position_induced_transformer_amd import metric, ops
    g = torch.Generator().manual_seed(n + j)
    mo = (torch.randint(0, 1024, (n, len(per)), generator=g).float() / 1024.0).cuda()
    mi = (torch.randint(0, 1024, (j, len(per)), generator=g).float() / 1024.0).cuda()
    wraps = any(p is not None for p in per)
    sq = metric.sqdist_periodic_box(per) if wraps else metric.sqdist_euclid
    ref = metric.knn_lists(sq, mo, mi, k)
    for got in (metric.knn_lists_box(mo, mi, k, periods=per if wraps else None), metric.knn_lists(sq, mo, mi, k, select="hip")):
        assert got.idx.shape == ref.idx.shape == (n, k) and got.idx.dtype == ref.idx.dtype
        assert torch.equal(got.sqd.sort(-1).values, ref.sqd.sort(-1).values)
        assert bool((got.sqd[:, 1:] >= got.sqd[:, :-1]).all())                     # the lists come ascending
        assert int(got.cut_rows) == int(ref.cut_rows)
        raw = ops.knn_box(mo, mi, k, per if wraps else None)
        assert torch.equal(raw.dist, got.sqd)                                      # exact arithmetic: the kernel's values are sqdist's
        tied = raw.next == raw.dist[:, -1]                                         # pair k + 1 no farther than pair k
        print("rows tied at the cut:", int(tied.sum()), "of", n)
        assert int(tied.sum()) <= 0.05 * n
        assert torch.equal(got.idx[~tied].sort(-1).values, ref.idx[~tied].sort(-1).values)


@pytest.mark.parametrize("out_batched,in_batched", [(True, True), (True, False), (False, True)])
def test_chunked_rows_builder_on_batched_meshes_is_the_box_builder(out_batched, in_batched):
    """select='hip' over several chunks of rows (the last one short) and a batch: the lists, distances and cut_rows of the box
    entry on a lattice with many exact ties (64 steps per axis), where the cut falls inside a tie shell on some rows."""
    from position_induced_transformer_amd import metric
    g = torch.Generator().manual_seed(17)
    mo = torch.randint(0, 64, (3, 130, 2) if out_batched else (130, 2), generator=g).float().div(64.0).cuda()
    mi = torch.randint(0, 64, (3, 300, 2) if in_batched else (300, 2), generator=g).float().div(64.0).cuda()
    per = (1.0, None)
    box = metric.knn_lists_box(mo, mi, 24, periods=per, locality=0.05)
    rows = metric.knn_lists(metric.sqdist_periodic_box(per), mo, mi, 24, chunk=48, locality=0.05, select="hip")
    assert box.idx.shape == (3, 130, 24) and torch.equal(rows.idx, box.idx) and torch.equal(rows.sqd, box.sqd)
    assert int(rows.cut_rows) == int(box.cut_rows)
    ref = metric.knn_lists(metric.sqdist_periodic_box(per), mo, mi, 24, chunk=48, locality=0.05)
    assert int(ref.cut_rows) == int(box.cut_rows) and torch.equal(ref.sqd.sort(-1).values, box.sqd)


def test_listed_distances_carry_mesh_gradients():
    from position_induced_transformer_amd import metric
    g = torch.Generator().manual_seed(9)
    mo = torch.rand(2, 40, 2, generator=g).cuda().requires_grad_(True)
    mi = torch.rand(90, 2, generator=g).cuda().requires_grad_(True)
    per = (1.0, None)
    lists = metric.knn_lists_box(mo, mi, 12, periods=per, locality=0.05)
    assert lists.idx.shape == (2, 40, 12) and lists.sqd.requires_grad and not lists.idx.requires_grad
    lists.sqd.sum().backward()
    mo2, mi2 = mo.detach().clone().requires_grad_(True), mi.detach().clone().requires_grad_(True)
    torch.gather(metric.sqdist_periodic_box(per)(mo2, mi2), -1, lists.idx).sum().backward()
    assert _err(mo.grad, mo2.grad) <= 1e-6 and _err(mi.grad, mi2.grad) <= 1e-6


# --------------------------------------------------------------------------- 5. determinism and capture
@pytest.mark.parametrize("j,k", [(700, 48), (2 * R + 37, 200)])
def test_two_runs_give_the_same_bits(j, k):
    from position_induced_transformer_amd import ops
    mo, mi = _cloud(41, 2, 67, 3, "random", True).cuda(), _cloud(42, 2, j, 3, "twice", True).cuda()
    a = ops.knn_box(mo, mi, k, (1.0, None, None))
    b = ops.knn_box(mo, mi, k, (1.0, None, None))
    _same_bits(a, type(b)(*(t.cpu() for t in b)), (j, k))


@pytest.mark.parametrize("j,k", [(300, 40), (R + 100, 64)])
def test_a_captured_call_replays_on_new_coordinates(j, k):
    from position_induced_transformer_amd import ops
    per = (None, 0.75)
    clouds = [(_cloud(50 + t, 2, 37, 2, "random", True), _cloud(60 + t, 1, j, 2, "twice" if t == 1 else "random", False)[0])
              for t in range(3)]
    mo, mi = clouds[0][0].cuda(), clouds[0][1].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.knn_box(mo, mi, k, per)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.knn_box(mo, mi, k, per)
    for t in (1, 2, 0):
        mo.copy_(clouds[t][0]); mi.copy_(clouds[t][1])
        graph.replay()
        _same_bits(res, ops.knn_box_restated(clouds[t][0], clouds[t][1], k, per), (j, k, t))


# --------------------------------------------------------------------------- 6. memory
def test_a_large_call_allocates_its_outputs_only():
    """N = J = 32 768, k = 32: the lists are 8 MiB; one block of the chunked builder (4096 rows x J) is 512 MiB."""
    from position_induced_transformer_amd import ops
    n = j = 32768
    k = 32
    g = torch.Generator().manual_seed(77)
    mo, mi = torch.rand(n, 2, generator=g), torch.rand(j, 2, generator=g)
    mo_d, mi_d = mo.cuda(), mi.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = ops.knn_box(mo_d, mi_d, k)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    out_bytes = sum(t.numel() * t.element_size() for t in got)
    print("knn_box at 32768 x 32768, k 32: peak memory grew by", grew, "bytes; outputs", out_bytes)
    assert out_bytes == n * k * 8 + n * 4
    assert grew <= 2 * out_bytes
    assert 4096 * j * 4 == 512 * 2 ** 20 and grew < 4096 * j * 4 // 16
    assert ops.knn_last_form() == 2
    rows = torch.arange(0, n, 2731)                                  # a dozen rows against the restatement
    ref = ops.knn_box_restated(mo[rows], mi, k)
    _same_bits(type(got)(got.idx[rows.cuda()], got.dist[rows.cuda()], got.next[rows.cuda()]), ref, "large")


# --------------------------------------------------------------------------- 7. the model
def _model_case(sqdist, learn_latent, seed):
    """tests/test_gpu_distlist.py's model, its seeds and shapes, with the lists built by the HIP builder."""
    from position_induced_transformer_amd import metric
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ltt = orc.grid_mesh_2d(16, False) + (0.01 * torch.rand(256, 2, generator=g) if learn_latent else 0.0)
    model = metric.pit_metric(2, 1, 1, 64, 2, 2, ltt, 0.05, 0.05, sqdist=sqdist, learn_latent=learn_latent, neighbors="auto",
                              builder="hip").cuda()
    mesh_in, mesh_out = torch.rand(700, 2, generator=g), torch.rand(900, 2, generator=g)
    return model, mesh_in, mesh_out, torch.randn(2, 700, 1, generator=g)


def test_model_with_the_hip_builder_matches_the_oracle(monkeypatch):
    from position_induced_transformer_amd import metric, ops
    from test_gpu_distlist import _model_oracle
    from test_gpu_models import TOL_GRAD, TOL_HEAD, TOL_OUT
    model, mesh_in, mesh_out, f = _model_case(metric.sqdist_euclid, False, 111)
    log = LaunchLog(monkeypatch)
    with ops.head_scale_route("host"):
        out = model(mesh_in.cuda(), f.cuda(), mesh_out.cuda())
        assert log.count("pit_knn_box") == 2 and log.count("pit_knn_rows") == 0, log.calls
        out.square().sum().backward()
    assert int(model.down.last_lists.cut_rows) == 0 and int(model.up.last_lists.cut_rows) == 0
    assert model.down.last_lists.idx.shape == (256, metric.default_neighbors(0.05, 700))
    assert model.up.last_lists.idx.shape == (900, metric.default_neighbors(0.05, 256))
    assert not [c for c in log.calls if c.startswith(FUSED)], log.calls
    assert log.count("pit_distlist_fwd") == 2 and log.count("pit_distlist_bwd") == 2 and log.count("pit_distmat_fwd") == 2
    assert log.count("pit_knn_box") == 2
    ref, p64, _ = _model_oracle(model, metric.sqdist_euclid, mesh_in, mesh_out, f, monkeypatch)
    assert gio.rel_l2(ref.numpy(), out.detach().double().cpu().numpy()) <= TOL_OUT
    for name, p in model.named_parameters():
        err = gio.rel_l2(p64[name].grad.numpy(), p.grad.double().cpu().numpy())
        print("model, hip builder", name, err)
        assert err <= (TOL_HEAD if name.endswith("lmda") else TOL_GRAD), (name, err)


def test_learnable_latent_mesh_with_the_hip_builder_under_a_periodic_box(monkeypatch):
    from position_induced_transformer_amd import metric, ops
    from test_gpu_distlist import _model_oracle
    from test_gpu_shared_latent import GRAD_TOL
    sq = metric.sqdist_periodic_box((1.0, None))
    model, mesh_in, mesh_out, f = _model_case(sq, True, 112)
    log = LaunchLog(monkeypatch)
    with ops.head_scale_route("host"):
        out = model(mesh_in.cuda(), f.cuda(), mesh_out.cuda())
        assert log.count("pit_knn_box") == 2 and log.count("pit_knn_rows") == 0, log.calls
        out.square().sum().backward()
    assert int(model.down.last_lists.cut_rows) == 0 and int(model.up.last_lists.cut_rows) == 0
    _, _, ltt64 = _model_oracle(model, sq, mesh_in, mesh_out, f, monkeypatch)
    err = _err(model.mesh_ltt.grad, ltt64.grad)
    print("latent mesh grad, hip builder", err)
    assert err <= GRAD_TOL


def test_any_other_metric_takes_the_rows_entry(monkeypatch):
    """A metric without box_periods: the chunks of knn_lists, selected by pit_knn_rows; the same lists as the box entry gives
    for the same distances (a lattice: exact)."""
    from position_induced_transformer_amd import metric
    g = torch.Generator().manual_seed(5)
    mo = (torch.randint(0, 1024, (2, 130, 2), generator=g).float() / 1024.0).cuda()
    mi = (torch.randint(0, 1024, (300, 2), generator=g).float() / 1024.0).cuda()
    layer = metric.posatt_cross_metric(2, 4, 0.05, lambda a, b: metric.sqdist_euclid(a, b), neighbors="auto", builder="hip").cuda()
    log = LaunchLog(monkeypatch)
    out = layer(mo, mi, torch.randn(2, 300, 4, generator=g).cuda())
    assert out.shape == (2, 130, 8) and log.count("pit_knn_rows") == 1 and log.count("pit_knn_box") == 0
    box = metric.knn_lists_box(mo, mi, None, locality=0.05)
    assert torch.equal(layer.last_lists.idx, box.idx) and torch.equal(layer.last_lists.sqd, box.sqd)
