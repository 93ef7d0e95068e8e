"""GPU: tasks.pit_cloud_fps - per-sample clouds on a latent mesh sampled from each cloud on the device - against the oracle
called ONCE PER SAMPLE on that sample's real points with the latent mesh ``cloud[ref_idx]``, ``ref_idx`` from the numpy
restatement of the sampler (tests/test_gpu_fps.py).  The convention and the tolerances of tests/test_gpu_ragged.py: fp32 oracle
and its fp64 evaluation with the kept sets of the fp32 twin; forward 1e-6, gradients 1e-5 of max|ref| per tensor, lmda 1e-4."""
import numpy as np
import pytest
import torch

import pit_oracle as orc
from test_gpu_fps import fps_reference, fps_reference_batch
from test_gpu_ragged import FWD_TOL, GRAD_TOL, LMDA_TOL, _check_predictions, _err, fp32_keep_oracle

pytestmark = pytest.mark.gpu
WIDTH, N_LATENT, BLOCKS = 150, 48, 2
BF16_OUT, BF16_GRAD, BF16_HEAD = 2e-2, 5e-2, 5e-2            # tests/test_gpu_bf16.py: relative L2


def _model(seed=3, hid=64):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    return tasks.pit_cloud_fps(2, 1, 1, hid, 2, BLOCKS, N_LATENT, 0.1, 0.2).cuda()


def _oracle(model, mesh, func, target, lengths, dtype, mesh_grad=False):
    """Per-sample oracle of the model + RelLpNorm(p=2): predictions, summed loss, summed parameter gradients (and d mesh)."""
    params = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in model.state_dict().items()}
    preds, loss, meshes = [], 0.0, []
    for s, n in enumerate(lengths):
        idx = fps_reference(mesh[s].numpy(), model.n_latent, n, model.start)[0]
        idx = torch.from_numpy(idx[idx >= 0].astype(np.int64))
        m = mesh[s:s + 1, :n].to(dtype).requires_grad_(mesh_grad)
        f, t = func[s:s + 1, :n].to(dtype), target[s:s + 1, :n].to(dtype)
        p = orc.pit_apply(params, "euclid", True, BLOCKS, model.en_local, model.de_local, m, f, m[:, idx], m)
        preds.append(p.detach())
        meshes.append(m)
        loss = loss + orc.rel_lp_loss(t, p, 1, 2)
    grads = torch.autograd.grad(loss, list(params.values()) + (meshes if mesh_grad else []))
    out = dict(zip(params.keys(), grads))
    if mesh_grad:
        out["mesh"] = torch.cat(grads[len(params):])
    return preds, loss.detach(), out


def _hip_step(model, mesh, func, target, lengths=None, mesh_grad=False):
    from position_induced_transformer_amd import utils
    for p in model.parameters():
        p.grad = None
    m = mesh.cuda().requires_grad_(mesh_grad)
    if lengths is None:
        pred = model(m, func.cuda(), m)
        loss = utils.RelLpNorm(1, 2)(target.cuda(), pred)
    else:
        pred = model(m, func.cuda(), m, len_in=lengths)
        loss = utils.RelLpNorm(1, 2)(target.cuda(), pred, lengths)
    loss.backward()
    grads = {k: v.grad.detach().cpu() for k, v in model.named_parameters()}
    if mesh_grad:
        grads["mesh"] = m.grad.detach().cpu()
    return pred.detach().cpu(), loss.detach().cpu(), grads


def _check_latent(model, mesh, lengths, ragged, lat=None):
    """model.last_latent (or ``lat``, the result a captured graph writes) is the sampler's result on this batch, bit for bit."""
    ridx, rmesh, rlen = fps_reference_batch(mesh.numpy(), model.n_latent, lengths if ragged else None, model.start)
    lat = model.last_latent if lat is None else lat
    assert np.array_equal(lat.idx.cpu().numpy(), ridx)
    assert np.array_equal(lat.mesh.cpu().numpy().view(np.uint32), rmesh.view(np.uint32))
    if ragged:
        assert np.array_equal(lat.lengths.cpu().numpy(), rlen)
    else:
        assert lat.lengths is None


def _check_model(model, mesh, func, target, lengths, ragged, mesh_grad=False):
    pred, loss, grads = _hip_step(model, mesh, func, target, lengths if ragged else None, mesh_grad)
    _check_latent(model, mesh, lengths, ragged)
    ref32, _, _ = _oracle(model, mesh, func, target, lengths, torch.float32)
    with fp32_keep_oracle():
        ref64, loss64, rg = _oracle(model, mesh, func, target, lengths, torch.float64, mesh_grad)
    _check_predictions(pred, ref32, ref64, lengths)
    e = abs(float(loss) - float(loss64)) / abs(float(loss64))
    print(f"loss {float(loss):.7f} vs {float(loss64):.7f}: {e:.2e}")
    assert e <= FWD_TOL
    for k, gref in rg.items():
        e = _err(grads[k], gref.reshape(grads[k].shape))
        print(f"grad {k}: {e:.2e}")
        assert e <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), k


@pytest.mark.parametrize("lengths", [[150, 76, 101], [150, 76, 3]], ids=["mix", "one-shorter-than-n_latent"])
def test_ragged_model_vs_per_sample_oracle(lengths):
    from position_induced_transformer_amd import tasks
    model = _model()
    mesh, func, target, _ = tasks.ragged_clouds(lengths, WIDTH, seed=11, pad_value=float("nan"))
    _check_model(model, mesh, func, target, lengths, True)
    assert model.last_latent.lengths.tolist() == [min(N_LATENT, n) for n in lengths]


def test_full_width_without_lengths_fp32():
    from position_induced_transformer_amd import tasks
    model = _model()
    lengths = [WIDTH] * 3
    mesh, func, target, _ = tasks.ragged_clouds(lengths, WIDTH, seed=12)
    _check_model(model, mesh, func, target, lengths, False)


def _rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def test_full_width_without_lengths_bf16():
    from position_induced_transformer_amd import ops, tasks
    model = _model()
    lengths = [WIDTH] * 3
    mesh, func, target, _ = tasks.ragged_clouds(lengths, WIDTH, seed=12)
    with ops.math_mode("bf16"):
        pred, loss, grads = _hip_step(model, mesh, func, target)
    _check_latent(model, mesh, lengths, False)                    # (the sampler runs in fp32 in every math mode)
    ref, ref_loss, rg = _oracle(model, mesh, func, target, lengths, torch.float32)
    e = _rel_l2(pred, torch.cat(ref))
    print(f"bf16 prediction {e:.2e}")
    assert e <= BF16_OUT
    assert abs(float(loss) - float(ref_loss)) <= BF16_OUT * abs(float(ref_loss))
    heads_got, heads_ref = [], []
    for k, gref in rg.items():
        if k.endswith("lmda"):
            heads_got.append(grads[k].reshape(-1)); heads_ref.append(gref.reshape(-1))
            continue
        e = _rel_l2(grads[k], gref)
        print(f"bf16 grad {k}: {e:.2e}")
        assert e <= BF16_GRAD, k
    e = _rel_l2(torch.cat(heads_got), torch.cat(heads_ref))
    print(f"bf16 d(lmda) {e:.2e}")
    assert e <= BF16_HEAD


def test_mesh_gradient_flows_through_the_chosen_points():
    from position_induced_transformer_amd import tasks
    model = _model(hid=32)
    lengths = [WIDTH] * 2
    mesh, func, target, _ = tasks.ragged_clouds(lengths, WIDTH, seed=13)
    _check_model(model, mesh, func, target, lengths, False, mesh_grad=True)


# ----------------------------------------------------------------------------- captured steps
MIXES = ([150, 76, 101], [17, 150, 71], [48, 49, 3])
_STEPS = {}


def _train_step():
    if "train" not in _STEPS:
        from position_induced_transformer_amd import engine, tasks
        model = _model(hid=32)
        mesh, func, target, _ = tasks.ragged_clouds(MIXES[0], WIDTH, seed=20, device="cuda")
        step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, len_in=MIXES[0])
        step.capture(warmup=1)
        _STEPS["train"] = step
        _STEPS["latent"] = model.last_latent                       # the tensors the graph's sampler writes
        _STEPS["twin"] = _model(hid=32)                           # the same weights (same seed), for eager steps
    return _STEPS["train"]


@pytest.mark.parametrize("mix", [1, 2, 0])
def test_captured_train_step_serves_new_mixes(mix):
    """One capture; lengths, clouds and data overwritten through set_batch: the replay's prediction and loss equal an eager
    step's on the same data (1e-6), and the sampler inside the graph saw the new clouds."""
    from position_induced_transformer_amd import tasks
    step = _train_step()
    lengths = MIXES[mix]
    m, f, t, _ = tasks.ragged_clouds(lengths, WIDTH, seed=21 + mix, device="cuda", pad_value=float("nan"))
    step.set_batch(f, t, mesh_in=m, len_in=lengths)
    step.replay()
    torch.cuda.synchronize()
    out, loss = step.out.detach().cpu().clone(), float(step.loss)
    graph_grads = {k: q.grad.detach().cpu().clone() for k, q in step.model.named_parameters()}
    _check_latent(step.model, m.cpu(), lengths, True, _STEPS["latent"])
    pred, eager_loss, grads = _hip_step(_STEPS["twin"], m.cpu(), f.cpu(), t.cpu(), lengths)
    for s, n in enumerate(lengths):
        assert _err(out[s, :n], pred[s, :n]) <= FWD_TOL, s
    assert abs(loss - float(eager_loss)) <= FWD_TOL * abs(float(eager_loss))
    for k, g in grads.items():
        assert _err(graph_grads[k], g) <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), k


def test_captured_eval_step():
    from position_induced_transformer_amd import engine, tasks, utils
    model = _train_step().model
    mesh, func, target, _ = tasks.ragged_clouds(MIXES[0], WIDTH, seed=30, device="cuda")
    step = engine.EvalStep(model, (mesh, func, mesh, target), 1, 2, len_in=MIXES[0])
    step.capture(warmup=1)
    latent = model.last_latent
    step.reset()
    total = 0.0
    for i, lengths in enumerate(MIXES[1:]):
        m, f, t, _ = tasks.ragged_clouds(lengths, WIDTH, seed=31 + i, device="cuda", pad_value=float("nan"))
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
    assert res.count == 6 and abs(res.rel_lp - total) <= FWD_TOL * abs(total)
