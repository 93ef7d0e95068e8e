"""GPU: ragged and shared-latent cloud batches in engine.TrainStep, the one-launch ragged loss (pit_rel_lp_loss_ragged_fwd_grad) and
RelMaxNorm with lengths (pit_rel_max_norm_ragged).

Reference for every comparison: the oracle applied ONCE PER SAMPLE to that sample's first n_s points (orc.pit_apply,
orc.rel_lp_loss), evaluated in fp64 with the kept sets of its fp32 twin (fp32_keep_oracle) - the convention and the tolerances of
tests/test_gpu_ragged.py: forward and loss 1e-6, gradients 1e-5, lmda gradients 1e-4, after Adam steps 1e-4 (lmda 5e-4), each as
max|err| / max|ref| per tensor.  The one-launch loss is also held bit for bit to the two entries it replaces."""

import pytest
import torch

import pit_oracle as orc
from test_gpu_ragged import FWD_TOL, GRAD_TOL, LMDA_TOL, LaunchLog, _err, _hip_model_step, fp32_keep_oracle
from test_gpu_ragged import _oracle_model as _oracle_elasticity
from test_gpu_shared_latent import _latent
from test_gpu_shared_latent import _oracle_model as _oracle_latent

pytestmark = pytest.mark.gpu
# (batch, width, lengths): the second set covers the stride-256 edges and more than one pass
SHAPES = [(4, 70, [70, 1, 33, 64]), (4, 600, [600, 257, 256, 255])]
WIDTH, FIRST, SECOND = 100, [100, 52, 33], [17, 100, 71]
# The data seeds of the model tests.  A prediction is held to 1e-6 of the oracle's fp64 evaluation, which only says something about
# the kernels where the fp32 oracle itself is that close to it: for each set of lengths the seed is the first from 14 upwards at
# which the fp32 oracle is within 1e-6 of its fp64 evaluation on every sample (a property of the oracle and the data alone, found
# on the host: FIRST 14: 2.2e-6, 15: 1.01e-6, 16: 9.5e-7; SECOND 14: 1.3e-6, 15: 6.8e-7 - tests/test_gpu_ragged.py's seed).
SEED_FIRST, SEED_SECOND = 16, 15


def _series(shape, nch, seed, fill=0.0):
    b, width, lengths = shape
    g = torch.Generator().manual_seed(seed)
    true, pred = torch.full((b, width, nch), fill), torch.full((b, width, nch), fill)
    for s, n in enumerate(lengths):
        true[s, :n], pred[s, :n] = torch.randn(n, nch, generator=g), torch.randn(n, nch, generator=g)
    return true, pred


def _fused_loss(L, t, q, lens, p, ws, want_grad=True, clear=None, clear_n=0):
    b, width, nch = t.shape
    norms, loss = torch.full((b, nch, 2), -7.0, device="cuda"), torch.full((), -7.0, device="cuda")
    d = torch.full_like(q, -7.0) if want_grad else None
    rc = L.pit_rel_lp_loss_ragged_fwd_grad(t.data_ptr(), q.data_ptr(), lens.data_ptr(), b, width, nch, p, norms.data_ptr(),
                                           loss.data_ptr(), ws.data_ptr(), d.data_ptr() if want_grad else None,
                                           clear.data_ptr() if clear is not None else None, clear_n, None)
    assert rc == 0
    torch.cuda.synchronize()
    return norms, loss, d


def _two_entry_loss(L, t, q, lens, p):
    b, width, nch = t.shape
    norms, loss, d = torch.empty(b, nch, 2, device="cuda"), torch.empty((), device="cuda"), torch.full_like(q, -7.0)
    assert L.pit_rel_lp_loss_ragged_fwd(t.data_ptr(), q.data_ptr(), lens.data_ptr(), b, width, nch, p, norms.data_ptr(),
                                        loss.data_ptr(), None) == 0
    assert L.pit_rel_lp_loss_ragged_bwd(t.data_ptr(), q.data_ptr(), lens.data_ptr(), b, width, nch, p, norms.data_ptr(), None,
                                        d.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return norms, loss, d


# --------------------------------------------------------------------------- 1. the loss kernel
@pytest.mark.parametrize("shape", SHAPES, ids=["w70", "w600"])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("nch", [1, 3])
def test_loss_kernel_vs_fp64_and_the_two_entries(nch, p, shape):
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    b, width, lengths = shape
    true, pred = _series(shape, nch, 40 + 10 * nch + p)
    t, q = true.cuda(), pred.cuda()
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    norms, loss, d = _fused_loss(L, t, q, lens, p, ws)
    assert int(ws[0]) == 0                                           # the ticket is left zero
    # fp64: autograd of the truncated formula
    r = pred.double().requires_grad_(True)
    ref = sum(orc.rel_lp_loss(true[s:s + 1, :n].double(), r[s:s + 1, :n], nch, p) for s, n in enumerate(lengths))
    ref.backward()
    e_loss, e_grad = abs(float(loss) - float(ref)) / float(ref), _err(d, r.grad)
    print(f"nch {nch} p {p} width {width}: loss {e_loss:.2e} d_pred_unit {e_grad:.2e}")
    assert e_loss <= FWD_TOL
    assert e_grad <= GRAD_TOL
    for s, n in enumerate(lengths):
        assert torch.all(d[s, n:] == 0), f"sample {s}: padding"
    # the two entries it replaces: the same bits
    norms2, loss2, d2 = _two_entry_loss(L, t, q, lens, p)
    assert torch.equal(norms, norms2) and torch.equal(loss, loss2) and torch.equal(d, d2)
    # a second call on the same workspace, and one without the gradient
    norms3, loss3, d3 = _fused_loss(L, t, q, lens, p, ws)
    assert torch.equal(norms, norms3) and torch.equal(loss, loss3) and torch.equal(d, d3) and int(ws[0]) == 0
    norms4, loss4, _ = _fused_loss(L, t, q, lens, p, ws, want_grad=False)
    assert torch.equal(norms, norms4) and torch.equal(loss, loss4)


# --------------------------------------------------------------------------- 2. the clear
@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "odd-start"])
@pytest.mark.parametrize("clear_n", [0, 1, 1_000_003])
def test_clear_zeroes_exactly_clear_n_floats(clear_n, offset):
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    true, pred = _series(SHAPES[0], 1, 7)
    t, q = true.cuda(), pred.cuda()
    lens = torch.tensor(SHAPES[0][2], dtype=torch.int32, device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    buf = torch.ones(offset + clear_n + 1000, device="cuda")
    norms, loss, d = _fused_loss(L, t, q, lens, 2, ws, clear=buf[offset:], clear_n=clear_n)
    assert torch.all(buf[:offset] == 1) and torch.all(buf[offset:offset + clear_n] == 0) and torch.all(buf[offset + clear_n:] == 1)
    norms2, loss2, d2 = _two_entry_loss(L, t, q, lens, 2)
    assert torch.equal(norms, norms2) and torch.equal(loss, loss2) and torch.equal(d, d2)


# --------------------------------------------------------------------------- 3. padding
@pytest.mark.parametrize("shape", SHAPES, ids=["w70", "w600"])
def test_nan_padding_never_enters(shape):
    from position_induced_transformer_amd import _lib, utils
    L = _lib.lib()
    lens = torch.tensor(shape[2], dtype=torch.int32, device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    runs = []
    for fill in (0.0, float("nan")):
        true, pred = _series(shape, 3, 9, fill)
        t, q = true.cuda(), pred.cuda()
        with torch.no_grad():
            runs.append(_fused_loss(L, t, q, lens, 2, ws) + (utils.RelMaxNorm(3)(t, q, lens),))
    for a, b_, name in zip(runs[0], runs[1], ("norms", "loss", "d_pred_unit", "rel_max_norm")):
        assert torch.isfinite(b_).all(), name
        assert torch.equal(a, b_), name


# --------------------------------------------------------------------------- 4. RelMaxNorm with lengths
@pytest.mark.parametrize("shape", SHAPES, ids=["w70", "w600"])
@pytest.mark.parametrize("nch", [1, 3])
def test_rel_max_norm_with_lengths(monkeypatch, nch, shape):
    from position_induced_transformer_amd import utils
    b, width, lengths = shape
    true, pred = _series(shape, nch, 60 + nch)
    metric = utils.RelMaxNorm(nch)
    ref = sum(metric(true[s:s + 1, :n].double(), pred[s:s + 1, :n].double()) for s, n in enumerate(lengths))     # the host formula
    log = LaunchLog(monkeypatch)
    with torch.no_grad():
        for lens in (lengths, torch.tensor(lengths, device="cuda"), torch.tensor(lengths, dtype=torch.int32, device="cuda")):
            got = metric(true.cuda(), pred.cuda(), lens)
            e = abs(float(got) - float(ref)) / float(ref)
            print(f"nch {nch} width {width}: {e:.2e}")
            assert e <= FWD_TOL
        assert log.calls == ["pit_rel_max_norm_ragged"] * 3
        log.calls.clear()
        full = metric(true.cuda(), pred.cuda())                      # without lengths: the launch list is as before
        assert log.calls == ["pit_rel_max_norm"]
        assert abs(float(full) - float(metric(true, pred))) <= FWD_TOL * abs(float(full))


# --------------------------------------------------------------------------- 5 - 9. the step
def _elasticity(seed=3):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    return tasks.pit_elasticity(2, 1, 1, 32, 2, 2, None, 0.05, 0.05).cuda()


def _cloud_latent(seed=3):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    ltt = _latent(8, 8, torch.Generator().manual_seed(seed)).cuda()
    return tasks.pit_cloud_latent(2, 1, 1, 32, 2, 2, ltt, 0.05, 0.05).cuda()


MODELS = {"elasticity": (_elasticity, _oracle_elasticity), "cloud_latent": (_cloud_latent, _oracle_latent)}


def _check_step(step, oracle, mesh, func, target, lengths):
    """step.out / step.loss / the flat gradients against the per-sample oracle on (mesh, func, target)[: lengths]."""
    torch.cuda.synchronize()
    model = step.model
    mesh, func, target = mesh.cpu(), func.cpu(), target.cpu()
    ref32, _, _ = oracle(model, mesh, func, target, lengths, torch.float32)
    with fp32_keep_oracle():
        ref64, loss64, rg = oracle(model, mesh, func, target, lengths, torch.float64)
    pred = step.out.cpu()
    for s, n in enumerate(lengths):
        e64, e32, own = _err(pred[s, :n], ref64[s][0]), _err(pred[s, :n], ref32[s][0]), _err(ref32[s][0], ref64[s][0])
        print(f"sample {s} ({n} points): prediction vs fp64 oracle {e64:.2e}, vs fp32 oracle {e32:.2e} (fp32 oracle vs fp64 {own:.2e})")
        assert e64 <= FWD_TOL
        assert e32 <= FWD_TOL + own                                  # (the bound of test_gpu_ragged._check_predictions)
    e = abs(float(step.loss) - float(loss64)) / abs(float(loss64))
    print(f"loss {float(step.loss):.7f} vs {float(loss64):.7f}: {e:.2e}")
    assert e <= FWD_TOL
    for k, q in model.named_parameters():
        e = _err(q.grad, rg[k])
        print(f"grad {k}: {e:.2e}")
        assert e <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), k


def test_eager_step(monkeypatch):
    from position_induced_transformer_amd import engine, tasks
    model = _elasticity()
    mesh, func, target, _ = tasks.ragged_clouds(FIRST, WIDTH, seed=SEED_FIRST, device="cuda")
    step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, len_in=FIRST)
    assert step.len_in.dtype == torch.int32 and step.len_in.is_cuda and step.len_out is None
    step.flat.flat.fill_(123.0)                                      # the loss launch clears the flat buffer: no memset
    log = LaunchLog(monkeypatch)
    step.run_eager()
    _check_step(step, _oracle_elasticity, mesh, func, target, FIRST)
    assert log.calls.count("pit_rel_lp_loss_ragged_fwd_grad") == 1
    assert "pit_rel_lp_loss_ragged_fwd" not in log.calls and "pit_rel_lp_loss_ragged_bwd" not in log.calls
    assert not [c for c in log.calls if c.startswith("pit_rel_lp_loss_fwd")]
    assert "pit_posatt_ragged_fwd" in log.calls and "pit_posatt_ragged_bwd" in log.calls
    # the same bits as the hand-rolled step on a twin of the model (every sum of this path has a fixed order)
    twin = _elasticity()
    pred, loss, grads = _hip_model_step(twin, mesh, func, target, FIRST)
    assert torch.equal(step.out.cpu(), pred) and torch.equal(step.loss.cpu(), loss)
    for k, q in model.named_parameters():
        assert torch.equal(q.grad.cpu(), grads[k]), k


_CAPTURED = {}


def _captured(kind):
    """One captured step per model kind, shared by the tests below (no optimiser: the weights stay as they are)."""
    if kind not in _CAPTURED:
        from position_induced_transformer_amd import engine, tasks
        model = MODELS[kind][0]()
        mesh, func, target, _ = tasks.ragged_clouds(FIRST, WIDTH, seed=SEED_FIRST, device="cuda")
        step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, len_in=FIRST)
        step.capture(warmup=1)
        _CAPTURED[kind] = step
    return _CAPTURED[kind]


def _replay(step, lengths, seed, fill=0.0):
    from position_induced_transformer_amd import tasks
    m, f, t, _ = tasks.ragged_clouds(lengths, WIDTH, seed=seed, device="cuda", pad_value=fill)
    step.set_batch(f, t, mesh_in=m, len_in=lengths)
    step.replay()
    torch.cuda.synchronize()
    return m, f, t


@pytest.mark.parametrize("kind", list(MODELS))
def test_captured_step_serves_new_sizes(kind):
    step = _captured(kind)
    lens_before = step.len_in
    m, f, t = _replay(step, SECOND, SEED_SECOND)
    assert step.len_in is lens_before and step.len_in.tolist() == SECOND
    _check_step(step, MODELS[kind][1], m, f, t, SECOND)


@pytest.mark.parametrize("kind", list(MODELS))
def test_captured_step_never_reads_padding(kind):
    step = _captured(kind)
    lengths = [61, 2, 97]
    runs = []
    for fill in (0.0, float("nan")):
        _replay(step, lengths, 16, fill)
        runs.append((step.out.cpu().clone(), step.loss.cpu().clone(),
                     {k: q.grad.detach().cpu().clone() for k, q in step.model.named_parameters()}))
    (p0, l0, g0), (p1, l1, g1) = runs
    for s, n in enumerate(lengths):
        assert torch.isfinite(p1[s, :n]).all() and torch.equal(p0[s, :n], p1[s, :n]), f"sample {s}"
    assert torch.isfinite(l1) and torch.equal(l0, l1)
    diff = {}
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        if not torch.equal(g0[k], g1[k]):
            diff[k] = float((g0[k] - g1[k]).abs().max() / g0[k].abs().max())
    print("gradients not bit-identical:", diff)
    if kind == "elasticity":                                         # every sum of the ragged path has a fixed order
        assert not diff, diff


def test_adam_in_the_graph_follows_the_oracle():
    from position_induced_transformer_amd import engine, ops, tasks
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    lengths, width = [90, 41, 64], 90
    model = _elasticity()
    mesh, func, target, _ = tasks.ragged_clouds(lengths, width, seed=12)
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ropt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = FlatAdam(flat, lr=1e-3, zero_grads=True)
    clouds = mesh.cuda()                                             # mesh_out IS mesh_in: the loss runs over len_in
    step = engine.TrainStep(model, (clouds, func.cuda(), clouds, target.cuda()), 1, 2, optimizer=opt, flat=flat, len_in=lengths)
    assert step._len_loss is step.len_in
    start = flat.flat_params.clone()
    step.capture(warmup=1)                                           # (the warm-up step is an Adam step: undone below)
    torch.cuda.synchronize()
    flat.flat_params.copy_(start)
    for state in (opt.exp_avg, opt.exp_avg_sq, opt.step_count, flat.flat):
        state.zero_()
    ops.parameters_changed()
    for _ in range(3):
        step.replay()
        ropt.zero_grad()
        with fp32_keep_oracle():
            loss = 0.0
            for s, n in enumerate(lengths):
                m = mesh[s:s + 1, :n].double()
                p = orc.pit_apply(ref, "euclid", True, 2, model.en_local, model.de_local, m, func[s:s + 1, :n].double(), m, m)
                loss = loss + orc.rel_lp_loss(target[s:s + 1, :n].double(), p, 1, 2)
            loss.backward()
        ropt.step()
    torch.cuda.synchronize()
    assert int(opt.step_count) == 3 and float(flat.flat.abs().max()) == 0.0
    for k, v in model.state_dict().items():
        e = _err(v, ref[k])
        print(f"{k}: {e:.2e}")
        assert e <= (5e-4 if k.endswith("lmda") else 1e-4), k


def test_a_step_without_lengths_calls_no_ragged_entry(monkeypatch):
    from position_induced_transformer_amd import engine, tasks
    model = _elasticity()
    mesh, func, target, _ = tasks.ragged_clouds([60, 60], 60, seed=16, device="cuda")
    step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2)
    assert step.len_in is None and step.len_out is None
    log = LaunchLog(monkeypatch)
    step.run_eager()
    torch.cuda.synchronize()
    assert log.calls and not [c for c in log.calls if "ragged" in c]
    assert log.calls.count("pit_rel_lp_loss_fwd_grad") == 1 and torch.isfinite(step.loss)
