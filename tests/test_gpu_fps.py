"""GPU: farthest-point sampling on the device (pit_fps / ops.farthest_point_sample) against a numpy restatement of the
semantics in include/pit_hip.h - exact equality of idx, out_len and the BITS of out_mesh, on every tier and wave edge, ties,
ragged mixes with NaN padding, start values, batches beyond the CU count, strided and batch-free meshes, repeated launches and a
captured graph whose inputs change between replays.

The restatement (``fps_reference``) is the specification: fp32 throughout, explicit sequential adds and ``e * e``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = np.float32


def fps_reference(cloud, m, length=None, start=0):
    """One cloud (n, space_dim) fp32 -> (idx (m,) int32, mesh (m, space_dim) fp32, out_len)."""
    cloud = np.asarray(cloud, dtype=F32)
    n, sd = cloud.shape
    big = n if length is None else min(max(int(length), 1), n)          # L: the real points
    pts = cloud[:big]
    idx = np.full((m,), -1, dtype=np.int32)
    out = np.zeros((m, sd), dtype=F32)
    dist = np.full((big,), np.inf, dtype=F32)
    cur = min(max(int(start), 0), big - 1)
    picks = min(m, big)
    for t in range(picks):
        idx[t] = cur
        out[t] = pts[cur]
        e = pts[:, 0] - pts[cur, 0]
        d = e * e
        for c in range(1, sd):
            e = pts[:, c] - pts[cur, c]
            d = d + e * e
        assert d.dtype == F32
        dist = np.minimum(dist, d)
        cur = int(np.argmax(dist))                       # (the first of the largest: the lowest index)
    return idx, out, picks


def fps_reference_batch(mesh, m, lengths=None, start=0):
    mesh = np.asarray(mesh, dtype=F32)
    b = mesh.shape[0]
    starts = [int(start)] * b if np.isscalar(start) else [int(v) for v in start]
    res = [fps_reference(mesh[s], m, None if lengths is None else lengths[s], starts[s]) for s in range(b)]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], dtype=np.int32))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def _check(res, ref, lengths_given):
    ridx, rmesh, rlen = ref
    assert res.idx.dtype == torch.int32 and res.mesh.dtype == torch.float32
    got_idx, got_mesh = res.idx.cpu().numpy(), res.mesh.cpu().numpy()
    assert got_idx.shape == ridx.shape and got_mesh.shape == rmesh.shape
    assert np.array_equal(got_idx, ridx), np.argwhere(got_idx != ridx)[:5]
    assert np.array_equal(_bits(got_mesh), _bits(rmesh))
    if lengths_given:
        assert res.lengths.dtype == torch.int32 and np.array_equal(res.lengths.cpu().numpy(), rlen)
    else:
        assert res.lengths is None


def _sample(mesh, m, lengths=None, start=0):
    from position_induced_transformer_amd import ops
    dev_start = start.cuda() if torch.is_tensor(start) else start
    return ops.farthest_point_sample(mesh.cuda(), m, lengths, dev_start)


def _rand(b, n, sd, seed):
    return torch.rand(b, n, sd, generator=torch.Generator().manual_seed(seed))


def _ms(n):
    """m in 1, 2, n where small, and a typical quarter."""
    ms = {1, min(2, n), max(1, n // 4)}
    if n <= 257:
        ms.add(n)
    return sorted(ms)


# ----------------------------------------------------------------------------- tiers and wave edges
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("sd", [1, 2, 3])
def test_tier_and_wave_edges(n, sd):
    mesh = _rand(2, n, sd, 1000 * sd + n)
    for m in _ms(n):
        _check(_sample(mesh, m), fps_reference_batch(mesh.numpy(), m), False)


@pytest.mark.parametrize("n,m", [(4096, 1), (4096, 2), (4096, 1024), (4097, 1), (4097, 2), (4097, 1024), (16384, 40)])
@pytest.mark.parametrize("sd", [1, 2, 3])
def test_large_tiers(n, m, sd):
    mesh = _rand(1, n, sd, 10 * sd + n)
    _check(_sample(mesh, m), fps_reference_batch(mesh.numpy(), m), False)


@pytest.mark.parametrize("n", [1, 2, 63, 65, 256, 257, 1024, 1025, 4096])
@pytest.mark.parametrize("sd", [5, 8])
def test_wide_coordinates(n, sd):
    mesh = _rand(2, n, sd, 77 * sd + n)
    for m in ([1, min(2, n), max(1, n // 4)] if n > 257 else _ms(n)):
        _check(_sample(mesh, m), fps_reference_batch(mesh.numpy(), m), False)


def test_four_coordinates_and_last_point_of_the_tiers():
    """space_dim 4, 6, 7 (the other widths of the 8-coordinate instances), and the farthest point in the LAST slot of a tier."""
    for sd in (4, 6, 7):
        mesh = _rand(2, 300, sd, sd)
        _check(_sample(mesh, 75), fps_reference_batch(mesh.numpy(), 75), False)
    for n in (1024, 4096, 16384):
        mesh = _rand(1, n, 2, n) * 0.5
        mesh[0, n - 1] = torch.tensor([3.0, 3.0])
        res = _sample(mesh, 3)
        assert int(res.idx[0, 1]) == n - 1
        _check(res, fps_reference_batch(mesh.numpy(), 3), False)


# ----------------------------------------------------------------------------- ties
def _grid(side, sd=2):
    ax = torch.arange(side, dtype=torch.float32) / (side - 1)
    return torch.stack(torch.meshgrid(*([ax] * sd), indexing="ij"), -1).reshape(1, -1, sd)


def test_restatement_on_the_8x8_grid():
    idx, _, _ = fps_reference(_grid(8)[0].numpy(), 5)
    assert idx.tolist() == [0, 63, 7, 56, 27]


@pytest.mark.parametrize("side,sd", [(8, 2), (33, 2), (70, 2), (11, 3), (300, 1)])
def test_regular_grids_every_pick_a_tie(side, sd):
    mesh = _grid(side, sd)
    m = min(mesh.shape[1], 200)
    _check(_sample(mesh, m), fps_reference_batch(mesh.numpy(), m), False)


def test_duplicated_blocks_and_identical_points():
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(50, 2, generator=g)
    dup = torch.cat((pts, pts[:30], pts[10:50], pts[:1].expand(180, 2))).unsqueeze(0)        # 300 points, 50 distinct
    res = _sample(dup, 120)
    _check(res, fps_reference_batch(dup.numpy(), 120), False)
    assert sorted(res.idx[0, :50].tolist()) == list(range(50)) and res.idx[0, 50:].tolist() == [0] * 70
    same = torch.full((3, 1100, 3), 0.375)
    res = _sample(same, 64, start=5)
    _check(res, fps_reference_batch(same.numpy(), 64, start=5), False)
    assert res.idx[:, 0].tolist() == [5, 5, 5] and torch.all(res.idx[:, 1:] == 0)


# ----------------------------------------------------------------------------- ragged mixes, guards, start
def _lengths(kind, n, b):
    """The mixes of tests/test_gpu_ragged.py: full width, about half, not multiples of 16 / 64, very short clouds."""
    base = {"mix": [n, max(1, n // 2 + 1), 3, max(1, n - 7), 2], "one": [1, n, max(1, n // 3)], "full": [n] * b}[kind]
    return [min(n, v) for v in (base * b)[:b]]


def _nan_padded(b, n, sd, lengths, seed):
    mesh = torch.full((b, n, sd), float("nan"))
    g = torch.Generator().manual_seed(seed)
    for s, ns in enumerate(lengths):
        mesh[s, :ns] = torch.rand(ns, sd, generator=g)
    return mesh


@pytest.mark.parametrize("n,m,sd,kind", [(150, 48, 2, "mix"), (150, 48, 3, "one"), (1025, 300, 2, "mix"), (4100, 64, 3, "mix"),
                                         (600, 600, 1, "mix"), (300, 100, 5, "mix"), (64, 64, 2, "full")])
def test_ragged_mixes_with_nan_padding(n, m, sd, kind):
    b = 5
    lengths = _lengths(kind, n, b)
    mesh = _nan_padded(b, n, sd, lengths, n + sd)
    for lens in (lengths, torch.tensor(lengths, dtype=torch.int32).cuda(), torch.tensor(lengths, dtype=torch.int64)):
        res = _sample(mesh, m, lens)
        _check(res, fps_reference_batch(mesh.numpy(), m, lengths), True)
    assert torch.isfinite(res.mesh).all()
    for s, ns in enumerate(lengths):
        assert torch.all(res.idx[s, min(m, ns):] == -1) and torch.all(res.mesh[s, min(m, ns):] == 0)


def test_lengths_outside_the_width_are_clamped():
    mesh = _rand(4, 90, 2, 5)
    res = _sample(mesh, 30, torch.tensor([0, -4, 91, 100000], dtype=torch.int32).cuda())
    _check(res, fps_reference_batch(mesh.numpy(), 30, [1, 1, 90, 90]), True)


def test_guard_regions_keep_their_fill():
    """The raw entry on caller-owned buffers with a guard region behind each output (and before it)."""
    from position_induced_transformer_amd import _lib
    b, n, sd, m, guard = 5, 333, 3, 100, 64
    lengths = _lengths("mix", n, b)
    mesh = _nan_padded(b, n, sd, lengths, 9).cuda()
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    idx = torch.full((guard + b * m + guard,), -77, dtype=torch.int32).cuda()
    out = torch.full((guard + b * m * sd + guard,), -55.5).cuda()
    olen = torch.full((guard + b + guard,), -33, dtype=torch.int32).cuda()
    rc = _lib.lib().pit_fps(mesh.data_ptr(), b, n, sd, n * sd, lens.data_ptr(), None, 0, m, idx.data_ptr() + 4 * guard,
                            out.data_ptr() + 4 * guard, olen.data_ptr() + 4 * guard, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    ridx, rmesh, rlen = fps_reference_batch(mesh.cpu().numpy(), m, lengths)
    assert np.array_equal(idx[guard:-guard].cpu().numpy().reshape(b, m), ridx)
    assert np.array_equal(_bits(out[guard:-guard].cpu().numpy().reshape(b, m, sd)), _bits(rmesh))
    assert np.array_equal(olen[guard:-guard].cpu().numpy(), rlen)
    for t, fill in ((idx, -77), (out, -55.5), (olen, -33)):
        assert torch.all(t[:guard] == fill) and torch.all(t[-guard:] == fill)


def test_scalar_and_per_sample_start_clamped():
    b, n, m = 5, 200, 40
    lengths = [200, 101, 3, 193, 2]
    mesh = _nan_padded(b, n, 2, lengths, 21)
    for start in (0, 7, 199, 5000, -3):
        _check(_sample(mesh, m, lengths, start), fps_reference_batch(mesh.numpy(), m, lengths, start), True)
    for dt in (torch.int32, torch.int64):
        starts = torch.tensor([199, 150, -1, 0, 1], dtype=dt)
        _check(_sample(mesh, m, lengths, starts), fps_reference_batch(mesh.numpy(), m, lengths, starts.tolist()), True)
    full = _rand(3, 70, 3, 22)
    _check(_sample(full, 20, None, torch.tensor([69, 70, 35])), fps_reference_batch(full.numpy(), 20, None, [69, 70, 35]), False)


# ----------------------------------------------------------------------------- batch, layouts
@pytest.mark.parametrize("b", [1, 5, 300])
def test_batches(b):
    n, m = 130, 33
    lengths = _lengths("mix", n, b)
    mesh = _nan_padded(b, n, 2, lengths, b)
    _check(_sample(mesh, m, lengths), fps_reference_batch(mesh.numpy(), m, lengths), True)


def test_batch_free_mesh():
    mesh = _rand(1, 500, 2, 31)[0]
    res = _sample(mesh, 125)
    ref = fps_reference(mesh.numpy(), 125)
    assert res.idx.shape == (125,) and res.mesh.shape == (125, 2) and res.lengths is None
    assert np.array_equal(res.idx.cpu().numpy(), ref[0]) and np.array_equal(_bits(res.mesh.cpu().numpy()), _bits(ref[1]))
    res = _sample(mesh, 125, [77], 3)
    ref = fps_reference(mesh.numpy(), 125, 77, 3)
    assert res.lengths.shape == () and int(res.lengths) == 77
    assert np.array_equal(res.idx.cpu().numpy(), ref[0]) and np.array_equal(_bits(res.mesh.cpu().numpy()), _bits(ref[1]))


def test_strided_batch_and_other_layouts():
    from position_induced_transformer_amd import ops
    b, n, sd, m = 4, 97, 3, 25
    wide = torch.full((b, n + 13, sd), float("nan")).cuda()
    data = _rand(b, n, sd, 41)
    wide[:, :n] = data.cuda()
    view = wide[:, :n]                                                       # batch stride (n + 13) * sd > n * sd: used in place
    assert not view.is_contiguous()
    ref = fps_reference_batch(data.numpy(), m)
    _check(ops.farthest_point_sample(view, m), ref, False)
    chans = torch.cat((data, torch.full((b, n, 2), float("nan"))), -1).cuda()
    _check(ops.farthest_point_sample(chans[..., :sd], m), ref, False)       # rows not contiguous: copied by the op
    _check(ops.farthest_point_sample(data.cuda().requires_grad_(True), m), ref, False)


# ----------------------------------------------------------------------------- repeatability, capture
def test_two_launches_give_identical_bits():
    mesh = _grid(40).expand(3, -1, -1).contiguous().cuda()
    from position_induced_transformer_amd import ops
    a, c = ops.farthest_point_sample(mesh, 400, [1600, 801, 1000]), ops.farthest_point_sample(mesh, 400, [1600, 801, 1000])
    assert torch.equal(a.idx, c.idx) and torch.equal(a.mesh.view(torch.int32), c.mesh.view(torch.int32)) and torch.equal(a.lengths, c.lengths)


def test_capture_sees_lengths_and_mesh_updated_in_place():
    from position_induced_transformer_amd import ops
    b, n, m = 4, 300, 80
    mixes = ([300, 151, 3, 293], [17, 300, 79, 2], [80, 81, 300, 1])
    meshes = [_nan_padded(b, n, 2, lens, 50 + i) for i, lens in enumerate(mixes)]
    mesh, lens = meshes[0].cuda(), torch.tensor(mixes[0], dtype=torch.int32).cuda()
    start = torch.zeros(b, dtype=torch.int32).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.farthest_point_sample(mesh, m, lens, start)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.farthest_point_sample(mesh, m, lens, start)
    for i in (1, 2, 0):
        mesh.copy_(meshes[i].cuda()); lens.copy_(torch.tensor(mixes[i], dtype=torch.int32)); start.fill_(i)
        graph.replay()
        torch.cuda.synchronize()
        _check(res, fps_reference_batch(meshes[i].numpy(), m, mixes[i], i), True)


def test_refusals_on_the_device():
    from position_induced_transformer_amd import ops
    mesh = torch.rand(2, 50, 2).cuda()
    with pytest.raises(ValueError, match="n_samples"):
        ops.farthest_point_sample(mesh, 51)
    with pytest.raises(ValueError, match="beyond"):
        ops.farthest_point_sample(torch.zeros(1, 16385, 2).cuda(), 4)
    with pytest.raises(ValueError, match="beyond"):
        ops.farthest_point_sample(torch.zeros(1, 4097, 4).cuda(), 4)
    with pytest.raises(ValueError, match="one entry per sample"):
        ops.farthest_point_sample(mesh, 5, torch.tensor([50, 50, 50], dtype=torch.int32).cuda())
