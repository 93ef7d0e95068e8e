"""GPU: the large farthest-point sampler (pit_fps_large / ops.farthest_point_sample_large) and tasks.pit_cloud_fps beyond the
single-launch sampler's envelope.  The specification is the numpy restatement of tests/test_gpu_fps.py (``fps_reference``); every
sampler comparison is EXACT - idx, out_len and the bits of out_mesh - at slice edges, with wide coordinates, on the library's
slices, against pit_fps where both apply, on ties across slices, ragged mixes with NaN padding, a dirty and a reused workspace,
strided / batch-free / large batches and a captured graph whose inputs change between replays.  The model is held to the
per-sample oracle at the tolerances of tests/test_gpu_cloud_fps.py."""
import numpy as np
import pytest
import torch

from test_gpu_cloud_fps import _check_latent, _check_model
from test_gpu_fps import _bits, _check, _grid, _nan_padded, _rand, fps_reference, fps_reference_batch
from test_gpu_mesh_grad import LaunchLog
from test_gpu_ragged import FWD_TOL, _err

pytestmark = pytest.mark.gpu


def _large(mesh, m, lengths=None, start=0, slice_points=0):
    from position_induced_transformer_amd import ops
    dev_start = start.cuda() if torch.is_tensor(start) else start
    return ops.farthest_point_sample_large(mesh.cuda(), m, lengths, dev_start, slice_points)


def _same_bits(a, c):
    assert torch.equal(a.idx, c.idx) and torch.equal(a.mesh.view(torch.int32), c.mesh.view(torch.int32))
    assert (a.lengths is None and c.lengths is None) or torch.equal(a.lengths, c.lengths)


# ----------------------------------------------------------------------------- slices
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513, 1025])
@pytest.mark.parametrize("sd", [1, 2, 3])
def test_slice_edges(n, sd):
    mesh = _rand(2, n, sd, 1000 * sd + n)
    ms = {1, min(2, n), max(1, n // 4)} | ({n} if n <= 257 else set())
    for m in sorted(ms):
        _check(_large(mesh, m, slice_points=256), fps_reference_batch(mesh.numpy(), m), False)


@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("sd", [4, 5, 8])
def test_wide_coordinates(n, sd):
    mesh = _rand(2, n, sd, 77 * sd + n)
    for m in (1, 2, n // 4):
        _check(_large(mesh, m, slice_points=256), fps_reference_batch(mesh.numpy(), m), False)


@pytest.mark.parametrize("n", [16384, 16385, 40000])
def test_default_slices(n):
    mesh = _rand(1, n, 3, n)
    _check(_large(mesh, 40), fps_reference_batch(mesh.numpy(), 40), False)


def test_default_slices_ragged_beyond_the_small_envelope():
    lengths = [70000, 16390]
    mesh = _nan_padded(2, 70000, 2, lengths, 70)
    res = _large(mesh, 300, lengths)
    _check(res, fps_reference_batch(mesh.numpy(), 300, lengths), True)
    assert torch.isfinite(res.mesh).all()


@pytest.mark.parametrize("n", [972, 4097, 16384])
def test_same_bits_as_the_single_launch_sampler(n):
    from position_induced_transformer_amd import ops
    b, m = 2, 64
    lengths = [n, n // 2 + 3]
    mesh = _nan_padded(b, n, 2, lengths, n).cuda()
    full = _rand(b, n, 3, n + 1).cuda()
    for cloud, lens in ((full, None), (mesh, lengths)):
        small = ops.farthest_point_sample(cloud, m, lens, 7)
        for sp in (256, 0):
            _same_bits(ops.farthest_point_sample_large(cloud, m, lens, 7, sp), small)


# ----------------------------------------------------------------------------- ties across slices
def test_grid_every_pick_a_tie_across_slices():
    mesh = _grid(40)                                                   # 1600 points: 7 slices of 256
    res = _large(mesh, 20, slice_points=256)
    _check(res, fps_reference_batch(mesh.numpy(), 20), False)
    assert res.idx[0, :4].tolist() == [0, 1599, 39, 1560]


def test_coincident_points():
    same = torch.full((2, 600, 3), 0.375)
    res = _large(same, 5, start=300, slice_points=256)
    _check(res, fps_reference_batch(same.numpy(), 5, start=300), False)
    assert res.idx[:, 0].tolist() == [300, 300] and torch.all(res.idx[:, 1:] == 0)


@pytest.mark.parametrize("n,far", [(1000, 999), (1024, 1023), (1025, 1024), (1000, 512), (1000, 256)],
                         ids=["last-slot-partial-slice", "last-slot-full-slice", "slice-of-one-point", "first-slot-middle-slice",
                              "first-slot-second-slice"])
def test_farthest_point_at_a_slice_boundary(n, far):
    mesh = _rand(1, n, 2, n + far) * 0.5
    mesh[0, far] = torch.tensor([3.0, 3.0])
    res = _large(mesh, 3, slice_points=256)
    assert int(res.idx[0, 1]) == far
    _check(res, fps_reference_batch(mesh.numpy(), 3), False)


# ----------------------------------------------------------------------------- ragged
def test_ragged_with_nan_padding_and_starts_beyond_the_lengths():
    """L = 1, L < m, L on a slice edge (256) and one past it (257), slices wholly beyond L (all but the full cloud)."""
    n, m = 1000, 64
    lengths = [1000, 1, 256, 257, 30]
    mesh = _nan_padded(5, n, 2, lengths, 5)
    for lens in (lengths, torch.tensor(lengths, dtype=torch.int32).cuda()):
        res = _large(mesh, m, lens, slice_points=256)
        _check(res, fps_reference_batch(mesh.numpy(), m, lengths), True)
    assert torch.isfinite(res.mesh).all()
    for s, ns in enumerate(lengths):
        assert torch.all(res.idx[s, min(m, ns):] == -1) and torch.all(res.mesh[s, min(m, ns):] == 0)
    starts = torch.tensor([999, 5, 256, 255, -3], dtype=torch.int32)
    _check(_large(mesh, m, lengths, starts, 256), fps_reference_batch(mesh.numpy(), m, lengths, starts.tolist()), True)
    _check(_large(mesh, m, lengths, 5000, 256), fps_reference_batch(mesh.numpy(), m, lengths, 5000), True)


# ----------------------------------------------------------------------------- workspace
def test_dirty_and_reused_workspace_through_the_raw_entry():
    from position_induced_transformer_amd import _lib
    b, n, sd, m, sp = 3, 1025, 3, 50, 256
    lengths = [1025, 513, 40]
    mesh = _nan_padded(b, n, sd, lengths, 8).cuda()
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    size = _lib.lib().pit_fps_large_workspace(b, n, sp)
    assert size > 0
    work = torch.full((size,), 0xFF, dtype=torch.uint8).cuda()
    ref = fps_reference_batch(mesh.cpu().numpy(), m, lengths)
    results = []
    for _ in range(2):
        idx = torch.full((b, m), -77, dtype=torch.int32).cuda()
        out = torch.full((b, m, sd), -55.5).cuda()
        olen = torch.full((b,), -33, dtype=torch.int32).cuda()
        rc = _lib.lib().pit_fps_large(mesh.data_ptr(), b, n, sd, n * sd, lens.data_ptr(), None, 0, m, idx.data_ptr(), out.data_ptr(),
                                      olen.data_ptr(), sp, work.data_ptr(), _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), ref[0]) and np.array_equal(_bits(out.cpu().numpy()), _bits(ref[1]))
        assert np.array_equal(olen.cpu().numpy(), ref[2])
        results.append((idx, out))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1].view(torch.int32), results[1][1].view(torch.int32))


# ----------------------------------------------------------------------------- batch, layouts
def test_strided_batch():
    from position_induced_transformer_amd import ops
    b, n, sd, m = 4, 600, 3, 25
    wide = torch.full((b, n + 13, sd), float("nan")).cuda()
    data = _rand(b, n, sd, 41)
    wide[:, :n] = data.cuda()
    view = wide[:, :n]                                                       # batch stride (n + 13) * sd > n * sd: used in place
    assert not view.is_contiguous()
    _check(ops.farthest_point_sample_large(view, m, slice_points=256), fps_reference_batch(data.numpy(), m), False)


def test_batch_free_mesh():
    mesh = _rand(1, 700, 2, 31)[0]
    res = _large(mesh, 90, slice_points=256)
    ref = fps_reference(mesh.numpy(), 90)
    assert res.idx.shape == (90,) and res.mesh.shape == (90, 2) and res.lengths is None
    assert np.array_equal(res.idx.cpu().numpy(), ref[0]) and np.array_equal(_bits(res.mesh.cpu().numpy()), _bits(ref[1]))
    res = _large(mesh, 90, [77], 3, 256)
    ref = fps_reference(mesh.numpy(), 90, 77, 3)
    assert res.lengths.shape == () and int(res.lengths) == 77
    assert np.array_equal(res.idx.cpu().numpy(), ref[0]) and np.array_equal(_bits(res.mesh.cpu().numpy()), _bits(ref[1]))


def test_batch_of_300():
    b, n, m = 300, 600, 8
    lengths = ([600, 301, 3, 593, 2, 256, 257] * 43)[:b]
    mesh = _nan_padded(b, n, 2, lengths, b)
    _check(_large(mesh, m, lengths, slice_points=256), fps_reference_batch(mesh.numpy(), m, lengths), True)


# ----------------------------------------------------------------------------- capture
def test_capture_sees_cloud_lengths_and_start_updated_in_place():
    from position_induced_transformer_amd import ops
    b, n, m = 3, 1025, 32
    mixes = ([1025, 513, 3], [17, 1025, 256], [257, 31, 1025])
    meshes = [_nan_padded(b, n, 2, lens, 50 + i) for i, lens in enumerate(mixes)]
    mesh, lens = meshes[0].cuda(), torch.tensor(mixes[0], dtype=torch.int32).cuda()
    start = torch.zeros(b, dtype=torch.int32).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.farthest_point_sample_large(mesh, m, lens, start, 256)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.farthest_point_sample_large(mesh, m, lens, start, 256)
    for i in (1, 2, 0):
        mesh.copy_(meshes[i].cuda()); lens.copy_(torch.tensor(mixes[i], dtype=torch.int32)); start.fill_(300 * i)
        graph.replay()
        torch.cuda.synchronize()
        _check(res, fps_reference_batch(meshes[i].numpy(), m, mixes[i], 300 * i), True)


# ----------------------------------------------------------------------------- the model beyond the small envelope
WIDTH, N_LATENT = 17000, 48


def _model(n_latent=N_LATENT, seed=3):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    return tasks.pit_cloud_fps(2, 1, 1, 32, 2, 2, n_latent, 0.1, 0.2).cuda()


def test_ragged_model_vs_per_sample_oracle_at_width_17000():
    from position_induced_transformer_amd import tasks
    lengths = [17000, 9001]
    mesh, func, target, _ = tasks.ragged_clouds(lengths, WIDTH, seed=11, pad_value=float("nan"))
    _check_model(_model(), mesh, func, target, lengths, True)


def test_full_width_model_forward_and_latent_at_width_17000():
    import pit_oracle as orc
    from position_induced_transformer_amd import tasks
    model = _model()
    mesh, func, _, _ = tasks.ragged_clouds([WIDTH], WIDTH, seed=12)
    with torch.no_grad():
        pred = model(mesh.cuda(), func.cuda(), mesh.cuda()).cpu()
    _check_latent(model, mesh, [WIDTH], False)
    idx = torch.from_numpy(fps_reference(mesh[0].numpy(), N_LATENT)[0].astype(np.int64))
    params = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    from test_gpu_ragged import fp32_keep_oracle
    with fp32_keep_oracle(), torch.no_grad():
        m = mesh.double()
        ref = orc.pit_apply(params, "euclid", True, 2, model.en_local, model.de_local, m, func.double(), m[:, idx], m)
    e = _err(pred, ref)
    print(f"prediction vs fp64 oracle {e:.2e}")
    assert e <= FWD_TOL


def test_model_routes_by_width(monkeypatch):
    from position_induced_transformer_amd import tasks
    model = _model()
    log = LaunchLog(monkeypatch)
    for width, large, small in ((WIDTH, 1, 0), (150, 0, 1)):
        mesh, func, _, _ = tasks.ragged_clouds([width, width // 2], width, seed=13, device="cuda")
        log.calls.clear()
        with torch.no_grad():
            model(mesh, func, mesh, len_in=[width, width // 2])
        assert log.count("pit_fps_large") == large and log.count("pit_fps") == small, log.calls
        log.calls.clear()
        with torch.no_grad():
            model(mesh, func, mesh)
        assert log.count("pit_fps_large") == large and log.count("pit_fps") == small, log.calls


def test_captured_eval_step_at_width_16500():
    from position_induced_transformer_amd import engine, tasks, utils
    width, mixes = 16500, ([16500, 8000], [16385, 16500], [40, 12001])
    model = _model(n_latent=32)
    mesh, func, target, _ = tasks.ragged_clouds(mixes[0], width, seed=30, device="cuda")
    step = engine.EvalStep(model, (mesh, func, mesh, target), 1, 2, len_in=mixes[0])
    step.capture(warmup=1)
    latent = model.last_latent
    step.reset()
    total = 0.0
    for i, lengths in enumerate(mixes[1:]):
        m, f, t, _ = tasks.ragged_clouds(lengths, width, seed=31 + i, device="cuda", pad_value=float("nan"))
        step.set_batch(f, t, mesh_in=m, len_in=lengths)
        step.replay()
        torch.cuda.synchronize()
        _check_latent(model, m.cpu(), lengths, True, latent)
        with torch.no_grad():
            pred = model(m, f, m, len_in=lengths)
            total += float(utils.RelLpNorm(1, 2)(t, pred, lengths))
        for s, n in enumerate(lengths):
            assert _err(step.out[s, :n], pred[s, :n]) <= FWD_TOL, s
    res = step.result()
    assert res.count == 4 and abs(res.rel_lp - total) <= FWD_TOL * abs(total)
