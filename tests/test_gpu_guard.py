"""GPU: the guarded optimizer step (ddp.GuardedAdam over pit_adam_step_guarded; csrc/pit_optim.hip) - the gradient norm in
fp64 partials, the inert guard against ddp.FlatAdam bit for bit, clipping / AdamW / warm-up against torch on fp64 copies, the
skip of a non-finite gradient, the step inside a captured graph and on two data-parallel ranks.

Sizes follow test_gpu_reductions.py's Adam cases: n in {1, 255, 257, 262144, 262145, 600001}.  600001 takes a second trip of
the 2048-workgroup grid of the update; 262144 and 262145 sit on either side of the change of the norm's run length (1024 -> 2048
elements per partial, 256 -> 129 partials).

Bounds.  Norm: sqrt(sum(partials)) rounded to fp32 within 1.2e-7 relative of the fp64 norm of the same fp32 gradients - an
fp64 sum of at most 2^20 terms errs below 1e-9, then comes one rounding to fp32 (6e-8); the fp64 value itself (health().norm) is
held to that 1e-9.  The coefficient is an fp64 quotient rounded to fp32: 1.2e-7.  Parameters: the project's TOL_ADAM = 2e-6
rel-L2 against torch on fp64 copies; where torch's own fp32 Adam + clip_grad_norm_ is further than half of that from the fp64
run, twice that distance (measured in the test, on the CPU - the rule of test_gpu_reductions.py's instance-norm case).

The clip threshold.  Gradients are randn * step, and the threshold is meant to lie in the middle, so that early steps pass
unclipped and late ones clip.  The norm of the middle step itself would make that step's norm / max_norm exactly 1, the very
borderline the margin assertion (every ratio at least 1e-3 away from 1) excludes; the threshold is therefore the norm of one
more draw from the same generator scaled by 2.5, between the second and the third step.  The reference asserts the margin,
and that at least one step clips and one does not.
"""
import math
import os

import numpy as np
import pytest
import torch

import golden_io as gio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ADAM = 2e-6
LR, ETA_MIN, WD, B1, B2 = (float(np.float32(v)) for v in (1e-3, 1e-5, 1e-2, 0.8, 0.95))      # what the ABI's floats hold
T_MAX = 7
SIZES = [1, 255, 257, 262144, 262145, 600001]
STEPS = 5


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _optimizer(cls, p0, n, offset=0, **kw):
    """An optimizer of ``cls`` over one flat parameter of exactly n elements (FlatGradients pads to 16; cut back so that the
    kernels' tails are the ragged ones the size names).  ``offset`` = 1: the gradients live one word into an allocation whose
    neighbouring words hold NaN."""
    from position_induced_transformer_amd.ddp import FlatGradients
    gpu = torch.nn.Parameter(p0.cuda())
    flat = FlatGradients([gpu], flatten_params=True)
    flat.flat, flat.flat_params = flat.flat[:n], flat.flat_params[:n]
    if offset:
        room = torch.full((n + 2 * offset,), float("nan"), device="cuda")
        flat.flat = room[offset:offset + n]
        flat.flat.zero_()
        assert flat.flat.data_ptr() % 16 == 4 * offset and bool(torch.isnan(room[0])) and bool(torch.isnan(room[-1]))
    opt = cls(flat, lr=LR, betas=(B1, B2), eps=1e-8, eta_min=ETA_MIN, **kw)
    assert opt.exp_avg.numel() == n and flat.flat.numel() == n
    return opt, flat


def _gradients(n, seed=None):
    g = torch.Generator().manual_seed(n if seed is None else seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * float(step) for step in range(1, STEPS + 1)]
    middle = torch.randn(n, generator=g) * 2.5                      # the threshold's draw (module docstring)
    return p0, grads, float(middle.double().norm())


# --------------------------------------------------------------------------- the norm
@pytest.mark.parametrize("n", SIZES)
def test_norm_partials_fp64_fixed_bits_and_bounds(n):
    from position_induced_transformer_amd.ddp import GuardedAdam, guard_parts
    p0, grads, _ = _gradients(n)
    grad = grads[2]
    want = float(grad.double().norm())
    parts = guard_parts(n)
    seen = []
    for offset in (0, 1):
        opt, flat = _optimizer(GuardedAdam, p0, n, offset=offset, zero_grads=False)
        for call in range(2):
            flat.flat.copy_(grad.cuda())
            opt.partials.fill_(float("nan"))                          # what the launch does not write stays NaN
            opt.step()
            partials = opt.partials.clone()
            assert not bool(torch.isnan(partials[:parts]).any()) and bool(torch.isnan(partials[parts:]).all())
            got32 = float(torch.sqrt(partials[:parts].sum()).float())
            assert abs(got32 - want) <= 1.2e-7 * want, (n, offset, got32, want)
            seen.append(partials[:parts])
            health = opt.health()
            assert abs(health.norm - want) <= 1e-9 * want and health.skipped == 0 and health.calls == call + 1
            assert health.max_norm == health.norm and health.coef == 1.0 and health.clipped == 0
            assert torch.equal(flat.flat.cpu(), grad)                 # kept gradients are left alone
    # the same bits on two calls, and from the 16-byte and the dword loads (the same elements in the same places)
    assert all(_same_bits(seen[0], other) for other in seen[1:])
    print("norm", n, "parts", parts, "rel err fp32 %.2e" % (abs(got32 - want) / want))


# --------------------------------------------------------------------------- the inert guard is FlatAdam
@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep-grads", "zero-grads"])
@pytest.mark.parametrize("n", SIZES)
def test_inert_guard_equals_flat_adam_as_bits(n, zero_grads):
    """max_grad_norm=None, no warm-up, coupled decay, finite gradients: the guarded kernel multiplies by 1.0f and evaluates
    the rate through FlatAdam's expression - parameters, moments, step_count and scalars[0:3] are equal words."""
    from position_induced_transformer_amd.ddp import FlatAdam, GuardedAdam
    p0, grads, _ = _gradients(n)
    kw = dict(weight_decay=WD, cosine_t_max=T_MAX, zero_grads=zero_grads)
    plain, flat_a = _optimizer(FlatAdam, p0, n, **kw)
    guarded, flat_b = _optimizer(GuardedAdam, p0, n, **kw)
    for step, grad in enumerate(grads, start=1):
        for opt, flat in ((plain, flat_a), (guarded, flat_b)):
            flat.flat.copy_(grad.cuda())
            opt.step()
        assert int(plain.step_count) == int(guarded.step_count) == int(guarded.calls) == step
        assert _same_bits(flat_a.flat_params, flat_b.flat_params), step
        assert _same_bits(plain.exp_avg, guarded.exp_avg) and _same_bits(plain.exp_avg_sq, guarded.exp_avg_sq), step
        assert _same_bits(plain.scalars[:3], guarded.scalars[:3]), step
        assert int(_bits(guarded.scalars)[3]) == 0                    # the ticket word
        assert _same_bits(flat_a.flat, flat_b.flat)
        if zero_grads:
            assert not bool(_bits(flat_b.flat).any())
    health = guarded.health()
    assert (health.calls, health.applied, health.skipped, health.clipped) == (STEPS, STEPS, 0, 0)
    assert torch.isfinite(flat_b.flat_params).all()


# --------------------------------------------------------------------------- clipping, AdamW and warm-up against torch
def _torch_run(p0, grads, dtype, max_norm, decoupled, warmup, start, skip_at=None):
    """torch.optim.Adam / AdamW + clip_grad_norm_ + LambdaLR(guarded_lr) on a copy of p0 in ``dtype``: the parameters after
    every step and each step's (norm, coef).  ``skip_at``: that step calls scheduler.step() but not optimizer.step()."""
    from position_induced_transformer_amd.ddp import guarded_lr
    p = torch.nn.Parameter(p0.to(dtype).clone())         # (a copy also when dtype is p0's own)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=LR, betas=(B1, B2), eps=1e-8, weight_decay=WD)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: guarded_lr(e + 1, LR, ETA_MIN, T_MAX, warmup, start) / LR)
    params, looks = [], []
    for step, grad in enumerate(grads, start=1):
        if step != skip_at:
            p.grad = grad.to(dtype).clone()
            norm = float(grad.double().norm())
            if max_norm:
                torch.nn.utils.clip_grad_norm_([p], max_norm)
            looks.append((norm, min(1.0, max_norm / (norm + 1e-6)) if max_norm else 1.0))
            opt.step()
        else:
            looks.append(None)
        sched.step()
        params.append(p.detach().clone())
    return params, looks


@pytest.mark.parametrize("mode", ["adam-clip-keep-grads", "adamw-clip-warmup"])
@pytest.mark.parametrize("n", SIZES)
def test_clip_adamw_and_warmup_against_torch_fp64(n, mode):
    from position_induced_transformer_amd.ddp import GuardedAdam
    decoupled = mode.startswith("adamw")
    warmup, start = (2, 0.1) if decoupled else (0, 0.0)
    zero_grads = decoupled
    p0, grads, max_norm = _gradients(n, seed=n + 1)                   # (seed n + 1: at n = 1 both sides of the threshold occur)
    ref, looks = _torch_run(p0, grads, torch.float64, max_norm, decoupled, warmup, start)
    ratios = [norm / max_norm for norm, _ in looks]
    assert all(abs(r - 1.0) >= 1e-3 for r in ratios), ratios          # no borderline step hides a difference
    assert any(r < 1.0 for r in ratios) and any(r > 1.0 for r in ratios), ratios
    ref32, _ = _torch_run(p0, grads, torch.float32, max_norm, decoupled, warmup, start)
    opt, flat = _optimizer(GuardedAdam, p0, n, weight_decay=WD, cosine_t_max=T_MAX, zero_grads=zero_grads,
                           max_grad_norm=max_norm, decoupled=decoupled, warmup_steps=warmup, warmup_start=start)
    from position_induced_transformer_amd.ddp import guarded_lr
    clipped = 0
    for step, grad in enumerate(grads, start=1):
        flat.flat.copy_(grad.cuda())
        opt.step()
        norm, coef = looks[step - 1]
        clipped += coef < 1.0
        health = opt.health()
        assert abs(health.norm - norm) <= 1e-9 * norm, (step, health.norm, norm)
        assert abs(health.coef - coef) <= 1.2e-7 * coef, (step, health.coef, coef)
        assert (health.calls, health.applied, health.skipped, health.clipped) == (step, step, 0, clipped)
        want_lr = guarded_lr(step, LR, ETA_MIN, T_MAX, warmup, start)
        assert abs(float(opt.scalars[0]) - want_lr) <= 1.2e-7 * want_lr, (step, float(opt.scalars[0]), want_lr)
        if zero_grads:
            assert not bool(_bits(flat.flat).any())
        else:
            assert torch.equal(flat.flat.cpu(), grad)                 # kept gradients stay UNCLIPPED
        d32 = gio.rel_l2(ref[step - 1].numpy(), ref32[step - 1].numpy())
        tol = max(TOL_ADAM, 2.0 * d32)
        err = gio.rel_l2(ref[step - 1].numpy(), flat.flat_params.cpu().numpy())
        print("guard %s n=%d step %d: ratio %.3f torch fp32 %.2e -> bound %.2e; kernel %.2e" % (mode, n, step, ratios[step - 1], d32, tol, err))
        assert err <= tol, (step, err, tol)
    largest = max(norm for norm, _ in looks)
    assert abs(opt.health().max_norm - largest) <= 1e-9 * largest


# --------------------------------------------------------------------------- the skip
SECOND_TRIP = 2048 * 256 + 5
SKIP_CASES = [(n, where) for n in SIZES for where in sorted({0, n - 1})] + [(600001, SECOND_TRIP)]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("n,where", SKIP_CASES, ids=["n%d-at%d" % c for c in SKIP_CASES])
def test_non_finite_gradient_skips_the_step(n, where, bad):
    """One NaN / Inf in step 3 of 5: parameters, moments and step_count keep their bits, the gradients are cleared, the call
    is counted; steps 4 and 5 follow a torch run that called scheduler.step() but not optimizer.step() at step 3."""
    from position_induced_transformer_amd.ddp import GuardedAdam
    assert 0 <= where < n
    if where == SECOND_TRIP:
        assert where >= 2048 * 256                                    # an element of the update grid's second trip
    p0, grads, _ = _gradients(n)
    ref, _ = _torch_run(p0, grads, torch.float64, 0.0, False, 0, 0.0, skip_at=3)
    opt, flat = _optimizer(GuardedAdam, p0, n, weight_decay=WD, cosine_t_max=T_MAX, zero_grads=True)
    for step, grad in enumerate(grads, start=1):
        grad = grad.clone()
        if step == 3:
            grad[where] = bad
        before = [t.clone() for t in (flat.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_count)]
        flat.flat.copy_(grad.cuda())
        opt.step()
        after = (flat.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_count)
        health = opt.health()
        assert not bool(_bits(flat.flat).any()), step                 # cleared on every call, the skipped one included
        assert int(opt.calls) == health.calls == step
        if step == 3:
            assert all(_same_bits(a, b) for a, b in zip(before, after))
            assert health.skipped == 1 and health.applied == 2 and int(opt.step_count) == 2
            assert not math.isfinite(health.norm) and health.coef == 1.0
        else:
            assert health.skipped == (1 if step > 3 else 0) and int(opt.step_count) == health.applied == step - (step > 3)
            assert math.isfinite(health.norm)
        assert math.isfinite(health.max_norm)                         # the largest FINITE norm
        err = gio.rel_l2(ref[step - 1].numpy(), flat.flat_params.cpu().numpy())
        assert err <= TOL_ADAM, (step, err)
    print("skip", n, where, bad, "params %.2e" % err)


def test_a_skipped_step_leaves_kept_gradients_alone():
    from position_induced_transformer_amd.ddp import GuardedAdam
    n = 257
    p0, grads, _ = _gradients(n)
    opt, flat = _optimizer(GuardedAdam, p0, n, weight_decay=WD, zero_grads=False)
    grad = grads[0].clone()
    grad[100] = float("nan")
    flat.flat.copy_(grad.cuda())
    before = flat.flat_params.clone()
    opt.step()
    assert _same_bits(flat.flat.cpu(), grad) and _same_bits(before, flat.flat_params)
    assert opt.health().skipped == 1 and int(opt.step_count) == 0 and int(opt.calls) == 1


def test_a_huge_finite_gradient_is_clipped_not_skipped():
    """3e19 in every element: its square overflows fp32, its norm (4.8e20) does not - widened to fp64 before squaring."""
    from position_induced_transformer_amd.ddp import GuardedAdam
    n = 257
    p0, _, _ = _gradients(n)
    grad = torch.full((n,), 3e19)
    assert math.isinf(float((grad * grad).sum()))
    ref, looks = _torch_run(p0, [grad], torch.float64, 1.0, False, 0, 0.0)
    opt, flat = _optimizer(GuardedAdam, p0, n, weight_decay=WD, cosine_t_max=T_MAX, zero_grads=True, max_grad_norm=1.0)
    flat.flat.copy_(grad.cuda())
    opt.step()
    health = opt.health()
    norm, coef = looks[0]
    assert (health.applied, health.skipped, health.clipped) == (1, 0, 1) and int(opt.step_count) == 1
    assert abs(health.norm - norm) <= 1e-9 * norm and abs(health.coef - coef) <= 1.2e-7 * coef
    err = gio.rel_l2(ref[0].numpy(), flat.flat_params.cpu().numpy())
    assert torch.isfinite(flat.flat_params).all() and err <= TOL_ADAM, err


# --------------------------------------------------------------------------- in the graph
def _fixed_model(seed=3):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    model = tasks.pit_darcy(2, 1, 1, 16, 2, 2, tasks.grid_mesh_2d(4).cuda(), 0.2, 0.2).cuda()
    for name, q in model.named_parameters():
        if name.endswith("lmda"):
            q.requires_grad_(False)
    return model


def _fixed_data(n, seed=21):
    from position_induced_transformer_amd import tasks
    g = torch.Generator().manual_seed(seed)
    return tasks.grid_mesh_2d(6).cuda(), torch.randn(n, 6, 6, 1, generator=g).cuda(), torch.randn(n, 6, 6, 1, generator=g).cuda()


def test_captured_step_skips_a_nan_batch_and_goes_on():
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd.ddp import FlatGradients, GuardedAdam
    from position_induced_transformer_amd.engine import TrainStep
    mesh, x, y = _fixed_data(16)
    bad = y[8:12].clone()
    bad[1, 2, 3, 0] = float("nan")
    batches = [(x[4:8], y[4:8]), (x[8:12], bad), (x[12:16], y[12:16])]
    ends = []
    with ops.reproducible():
        for twin in range(2):
            model = _fixed_model()
            flat = FlatGradients(model.parameters(), flatten_params=True)
            opt = GuardedAdam(flat, lr=1e-3, cosine_t_max=10, zero_grads=True, max_grad_norm=0.5, warmup_steps=2, warmup_start=0.1)
            step = TrainStep(model, (mesh, x[:4].clone(), mesh, y[:4].clone()), 1, 2, optimizer=opt, flat=flat)
            step.capture()                                            # (three warm-up passes: real steps, the same for both twins)
            warm = step.health(reset=True)
            assert (warm.calls, warm.skipped, warm.finite_loss) == (3, 0, 3) and int(opt.calls) == 3
            losses, params = [], []
            for xb, yb in batches:
                step.set_batch(xb, yb)
                step.replay()
                losses.append(float(step.loss))
                params.append(flat.flat_params.clone())
            health = step.health()
            assert math.isfinite(losses[0]) and math.isnan(losses[1]) and math.isfinite(losses[2])
            assert _same_bits(params[0], params[1])                   # the NaN batch changed nothing
            assert not _same_bits(params[1], params[2]) and torch.isfinite(params[2]).all()
            assert (health.calls, health.applied, health.skipped) == (3, 2, 1) and int(opt.calls) == 6 and int(opt.step_count) == 5
            assert health.nonfinite_loss == 1 and health.finite_loss == 2
            want = math.fsum(v for v in losses if math.isfinite(v))
            assert abs(health.loss_sum - want) <= 1e-12 * abs(want) and abs(health.mean_loss - want / 2) <= 1e-12 * abs(want)
            assert not bool(_bits(flat.flat).any())                   # zero_grads: no NaN lives on in the accumulator
            ends.append((params[2], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), torch.tensor(losses)))
    for a, b in zip(*ends):
        assert _same_bits(a, b)                                       # a second model from the same seed: the same bits


# --------------------------------------------------------------------------- two ranks
def _guard_worker(rank, world, port, out_dir):
    import sys
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    for pth in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, pth)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from position_induced_transformer_amd.ddp import FlatGradients, GuardedAdam, broadcast_parameters, shard_batch
    from position_induced_transformer_amd.engine import TrainStep
    torch.cuda.set_device(0)                              # both ranks share the one GPU of the test box
    model = _fixed_model(seed=50 + rank)                  # different initialisations ...
    broadcast_parameters(model)                           # ... made rank 0's
    mesh, x, y = _fixed_data(12)
    sl = shard_batch(4, rank, world)
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = GuardedAdam(flat, lr=1e-3, cosine_t_max=10, zero_grads=True, max_grad_norm=0.5)
    step = TrainStep(model, (mesh, x[:4][sl].clone(), mesh, y[:4][sl].clone()), 1, 2, all_reduce=True, optimizer=opt, flat=flat)
    params = []
    for i in range(3):
        xb, yb = x[4 * i:4 * i + 4][sl].clone(), y[4 * i:4 * i + 4][sl].clone()
        if i == 1 and rank == 1:
            yb[0, 2, 3, 0] = float("nan")                 # one rank's shard alone carries the NaN
        step.set_batch(xb, yb)
        step.run_eager()
        torch.cuda.synchronize()
        params.append(flat.flat_params.cpu().numpy().view(np.int32).copy())
    health = step.health()
    np.save(os.path.join(out_dir, "params%d.npy" % rank), np.stack(params))
    np.save(os.path.join(out_dir, "health%d.npy" % rank), np.asarray([health.calls, health.applied, health.skipped,
                                                                       health.nonfinite_loss], dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decision(tmp_path):
    """Two processes share the GPU, gloo for the exchange (test_gpu_round2.py's data-parallel case).  The guard runs on the
    all-reduced buffer: rank 1's NaN skips step 2 on BOTH ranks, and the parameters are equal words after every step."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_guard_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    p0, p1 = (np.load(os.path.join(tmp_path, "params%d.npy" % r)) for r in (0, 1))
    h0, h1 = (np.load(os.path.join(tmp_path, "health%d.npy" % r)).tolist() for r in (0, 1))
    assert p0.shape == p1.shape and p0.shape[0] == 3 and np.array_equal(p0, p1)
    assert np.array_equal(p0[0], p0[1]) and not np.array_equal(p0[1], p0[2])          # step 2 changed nothing, step 3 did
    assert np.isfinite(p0.view(np.float32)).all()
    assert h0[:3] == h1[:3] == [3, 2, 1]
    assert (h0[3], h1[3]) == (0, 1)                       # the loss is each rank's own: only rank 1 saw a NaN loss
