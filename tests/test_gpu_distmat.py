"""GPU: position attention on caller-supplied squared distances (csrc/pit_distmat.hip, ops.DistPlan / posatt_dist_apply,
metric.py) against the oracle, which is already factored on the distance matrix: orc.attention_weights(m, c, q, batched) and
orc.weighted_values take m, not meshes.

Tolerances are the project's: forward 1e-6, 1e-5 per gradient tensor (test_gpu_mesh_grad.TOL), lmda gradients LMDA_TOL of
test_gpu_shared_latent; max |err| / max |ref| per tensor.  The fp64 oracle keeps the entries its fp32 twin keeps
(test_gpu_mesh_grad.fp32_keep_oracle); the head scale is on route 'host' (bit for bit pit.py:48 on the CPU) or injected."""
import pytest
import torch
import torch.nn as nn

import pit_oracle as orc
from test_gpu_mesh_grad import TOL, _err, fp32_keep_oracle
from test_gpu_shared_latent import FWD_TOL, LMDA_TOL

pytestmark = pytest.mark.gpu

# rows up to 2048 keys are searched in LDS (DM_SEL_LDS of csrc/pit_distmat.hip); J0 is a row the selection has to stream
J0 = 2100
SHAPES = [(1, 1), (33, 31), (100, 150), (8, J0)]
QS = [0.02, 0.05, 0.3, 1.0]


def _rand_m(shape, seed, dup=True):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(*shape, generator=g)
    if dup and shape[-1] > 4:                    # injected duplicates: tie shells at arbitrary ranks
        j = shape[-1]
        m[..., j // 3:j // 3 + j // 4] = m[..., j // 3:j // 3 + 1]
        m[..., -2] = m[..., 0]
    return m


def _grid_m():
    from position_induced_transformer_amd import metric
    mesh = orc.grid_mesh_2d(8, False)
    l = orc.period_2d(mesh)
    return metric.sqdist_periodic_box((l, l))(mesh, mesh)


# --------------------------------------------------------------------------- 1. selection
def _check_stats(m_dev, m_cpu, q):
    from position_induced_transformer_amd import ops
    plan = ops.DistPlan(m_dev, q)
    ref = orc.row_order_stats(m_cpu, q)
    got = plan.stats.cpu().reshape(3, -1)
    for i in range(3):
        assert torch.equal(got[i], ref[i].reshape(-1)), (tuple(m_cpu.shape), q, i)
    return plan


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{j}" for n, j in SHAPES])
def test_selection_is_exact(shape, q):
    n, j = shape
    shared = _rand_m((n, j), 1)
    plan = _check_stats(shared.cuda(), shared, q)
    assert plan.m_bstride == 0 and plan.m.data_ptr() == plan.source.data_ptr()       # a view, no copy
    per = _rand_m((3, n, j), 2)
    _check_stats(per.cuda(), per, q)
    wide = torch.full((n, j + 5), -1.0)                  # a row view with ld_m > J: the columns beyond are never read
    wide[:, :j] = shared
    view = wide.cuda()[:, :j]
    plan = _check_stats(view, shared, q)
    assert plan.ld_m == (j + 5 if n > 1 else j) and plan.m.data_ptr() == view.data_ptr()      # (one row: no row stride)


@pytest.mark.parametrize("q", QS)
def test_selection_is_exact_on_the_tie_shells_of_a_periodic_grid(q):
    m = _grid_m()
    _check_stats(m.cuda(), m, q)


# --------------------------------------------------------------------------- 2. the kept set
@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("shape", SHAPES + [(64, 64)], ids=[f"{n}x{j}" for n, j in SHAPES] + ["grid8x8"])
def test_kept_set_is_the_fp32_oracles(shape, q):
    from position_induced_transformer_amd import metric, ops
    torch.manual_seed(3)
    m = _grid_m() if shape == (64, 64) else _rand_m(shape, 4)
    mod = metric.posatt_cross_metric(2, shape[1], q).cuda()
    ref = orc.attention_weights(m, orc.head_scale(mod.lmda.detach().cpu()), q, False)
    with ops.head_scale_route("host"), torch.no_grad():
        att = mod.dist2att(m.cuda(), mod.lmda, q)
    assert att.shape == ref.shape
    assert torch.equal(att.cpu() != 0, ref != 0)
    if shape[0] * shape[1] <= 100 * 150:                 # ... and per sample
        mb = _rand_m((2,) + shape, 5)
        refb = orc.attention_weights(mb, orc.head_scale(mod.lmda.detach().cpu()), q, True)
        with ops.head_scale_route("host"), torch.no_grad():
            attb = mod.dist2att(mb.cuda(), mod.lmda, q)
        assert torch.equal(attb.cpu() != 0, refb != 0)


# --------------------------------------------------------------------------- 3. the layer matrix against fp64
# (heads, D, N, J, b, q); the self form takes J = N
CASES = [(1, 44, 100, 150, 3, 1.0), (2, 64, 70, 200, 1, 0.05), (2, 3, 130, 97, 3, 0.02), (1, 256, 50, 77, 3, 0.3),
         (2, 256, 200, 200, 3, 0.02)]


def _oracle_layer(m, x, dy, lmda, q, concat):
    """fp64 autograd through pit.py:48-57 on m."""
    lm = lmda.detach().double().cpu().requires_grad_(True)
    m64 = m.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    batched = m64.dim() == 3
    with fp32_keep_oracle():
        out = orc.weighted_values(orc.attention_weights(m64, orc.head_scale(lm), q, batched), x64, batched)
    if concat:
        out = torch.cat((x64, out), -1)
    out.backward(dy.double())
    return out, x64.grad, lm.grad, m64.grad


def _run_layer(mod, m, x, dy):
    from position_induced_transformer_amd import ops
    m1, x1 = m.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    mod.lmda.grad = None
    with ops.head_scale_route("host"):
        out = mod.forward_dist(m1, x1)
        out.backward(dy.cuda())
    return out, x1.grad, mod.lmda.grad.clone(), m1.grad


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-sample"])
@pytest.mark.parametrize("form", ["cross", "self"])
@pytest.mark.parametrize("case", CASES, ids=[f"h{c[0]}-d{c[1]}-{c[2]}x{c[3]}-b{c[4]}-q{c[5]}" for c in CASES])
def test_layer_matches_fp64(case, form, shared):
    from position_induced_transformer_amd import metric
    heads, dim, n, j, b, q = case
    concat = form == "self"
    if concat:
        j = n
    torch.manual_seed(CASES.index(case))
    g = torch.Generator().manual_seed(10 + CASES.index(case))
    mod = (metric.posatt_metric if concat else metric.posatt_cross_metric)(heads, dim, q).cuda()
    m = torch.rand(*((n, j) if shared else (b, n, j)), generator=g)
    x = torch.randn(b, j, dim, generator=g)
    dy = torch.randn(b, n, (heads + (1 if concat else 0)) * dim, generator=g)
    got = _run_layer(mod, m, x, dy)
    ref = _oracle_layer(m, x, dy, mod.lmda, q, concat)           # (a shared m64: autograd sums d_m over the samples)
    errs = {"out": _err(got[0], ref[0]), "d_values": _err(got[1], ref[1]), "d_lmda": _err(got[2].reshape(-1), ref[2].reshape(-1)),
            "d_m": _err(got[3], ref[3])}
    print(case, form, shared, errs)
    assert got[3].shape == m.shape
    assert errs["out"] <= FWD_TOL and errs["d_values"] <= TOL and errs["d_m"] <= TOL and errs["d_lmda"] <= LMDA_TOL, errs


# --------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-sample"])
def test_two_runs_give_the_same_bits(shared):
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(21)
    n, j, b = 130, 170, 3
    m = torch.rand(*((n, j) if shared else (b, n, j)), generator=g).cuda()
    x, dy = torch.randn(b, j, 48, generator=g).cuda(), torch.randn(b, n, 96, generator=g).cuda()
    c = torch.tensor([14.0, 9.0], device="cuda")
    runs = []
    for _ in range(2):
        m1, x1 = m.clone().requires_grad_(True), x.clone().requires_grad_(True)
        out = ops.posatt_dist_apply(x1, c, ops.DistPlan(m1, 0.1), 2, concat=False, head_is_scale=True, m_dist=m1)
        out.backward(dy)
        runs.append((out.detach().clone(), x1.grad.clone(), m1.grad.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


# --------------------------------------------------------------------------- 5. agreement with the built-in metrics
def test_periodic_box_agrees_with_the_periodic2d_layer():
    from position_induced_transformer_amd import metric
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(5)
    mesh = orc.grid_mesh_2d(16, False)
    l = orc.period_2d(mesh)
    sq = metric.sqdist_periodic_box((l, l))
    mod = metric.posatt_metric(2, 24, 0.05, sq).cuda()
    x, dy = torch.randn(2, 256, 24, generator=g), torch.randn(2, 256, 72, generator=g)
    got = _run_layer(mod, sq(mesh, mesh), x, dy)
    lm, x64 = mod.lmda.detach().double().cpu().requires_grad_(True), x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_self("periodic2d", False, mesh.double(), x64, lm, 0.05)
    ref.backward(dy.double())
    errs = (_err(got[0], ref), _err(got[1], x64.grad), _err(got[2].reshape(-1), lm.grad.reshape(-1)))
    print("periodic2d", errs)
    assert errs[0] <= FWD_TOL and errs[1] <= TOL and errs[2] <= LMDA_TOL, errs


def test_euclid_helper_agrees_with_the_euclidean_cross_layer():
    from position_induced_transformer_amd import metric
    torch.manual_seed(6)
    g = torch.Generator().manual_seed(6)
    mo, mi = torch.rand(2, 90, 3, generator=g), torch.rand(2, 140, 3, generator=g)
    mod = metric.posatt_cross_metric(2, 40, 0.1).cuda()
    x, dy = torch.randn(2, 140, 40, generator=g), torch.randn(2, 90, 80, generator=g)
    got = _run_layer(mod, metric.sqdist_euclid(mo, mi), x, dy)
    lm, x64 = mod.lmda.detach().double().cpu().requires_grad_(True), x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", True, mo.double(), mi.double(), x64, lm, 0.1)
    ref.backward(dy.double())
    errs = (_err(got[0], ref), _err(got[1], x64.grad), _err(got[2].reshape(-1), lm.grad.reshape(-1)))
    print("euclid", errs)
    assert errs[0] <= FWD_TOL and errs[1] <= TOL and errs[2] <= LMDA_TOL, errs


# --------------------------------------------------------------------------- 6. what the feature is for
def test_mesh_gradient_under_the_periodic_metric_matches_fp64():
    """mesh.grad under a periodic metric - refused by the built-in periodic layers - through autograd over the user's sqdist."""
    from position_induced_transformer_amd import metric, ops
    torch.manual_seed(7)
    g = torch.Generator().manual_seed(7)
    mesh_in = orc.grid_mesh_2d(16, False)                        # the period comes from this one (pit.py:248-250): 1.0
    mesh_out = torch.rand(120, 2, generator=g)                   # jittered points: no |dx| = l - |dx| tie
    l = orc.period_2d(mesh_in)
    mod = metric.posatt_cross_metric(2, 32, 0.05, metric.sqdist_periodic_box((l, l))).cuda()
    x, dy = torch.randn(3, 256, 32, generator=g), torch.randn(3, 120, 64, generator=g)
    mo1, x1 = mesh_out.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    with ops.head_scale_route("host"):
        out = mod(mo1, mesh_in.cuda(), x1)
        out.backward(dy.cuda())
    lm = mod.lmda.detach().double().cpu().requires_grad_(True)
    mo64, x64 = mesh_out.double().requires_grad_(True), x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("periodic2d", False, mo64, mesh_in.double(), x64, lm, 0.05)
    ref.backward(dy.double())
    errs = {"out": _err(out, ref), "d_mesh": _err(mo1.grad, mo64.grad), "d_values": _err(x1.grad, x64.grad),
            "d_lmda": _err(mod.lmda.grad.reshape(-1), lm.grad.reshape(-1))}
    print("periodic mesh grad", errs)
    assert errs["out"] <= FWD_TOL and errs["d_mesh"] <= TOL and errs["d_values"] <= TOL and errs["d_lmda"] <= LMDA_TOL, errs


def _box64(l):
    def sq(_metric, mo, mi):                                     # orc.sqdist_periodic2d with a GIVEN period
        d = abs(mo.unsqueeze(-2) - mi.unsqueeze(-3))
        d = torch.minimum(d, l - d)
        return torch.sum(d ** 2, dim=-1)
    return sq


def test_adam_on_a_learnable_latent_mesh_under_a_periodic_box_follows_fp64(monkeypatch):
    from position_induced_transformer_amd import metric, ops
    torch.manual_seed(8)
    g = torch.Generator().manual_seed(8)
    mesh = orc.grid_mesh_2d(12, False)
    ltt = orc.grid_mesh_2d(6, False) + 0.05 * torch.rand(36, 2, generator=g)
    model = metric.pit_metric(2, 1, 1, 32, 2, 2, ltt, 0.05, 0.05, sqdist=metric.sqdist_periodic_box((1.0, 1.0)), learn_latent=True).cuda()
    assert isinstance(model.mesh_ltt, nn.Parameter)
    f = torch.randn(2, 144, 1, generator=g)
    p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters() if k != "mesh_ltt"}
    ltt64 = model.mesh_ltt.detach().double().cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([model.mesh_ltt], lr=1e-3, eps=1e-3)
    opt64 = torch.optim.Adam([ltt64], lr=1e-3, eps=1e-3)
    monkeypatch.setattr(orc, "sqdist", _box64(1.0))
    for step in range(3):
        opt.zero_grad()
        with ops.head_scale_route("host"):
            model(mesh.cuda(), f.cuda(), mesh.cuda()).square().sum().backward()
        opt.step()
        opt64.zero_grad()
        with fp32_keep_oracle():
            orc.pit_apply(p64, "box", False, 2, 0.05, 0.05, mesh.double(), orc.with_coords(mesh.double(), f.double()), ltt64,
                          mesh.double()).square().sum().backward()
        opt64.step()
        err = float((model.mesh_ltt.detach().double().cpu() - ltt64.detach()).abs().max())
        print("adam box step", step, err)
        assert err <= 1e-5


def test_pit_metric_layers_are_foreign_to_the_fused_paths(monkeypatch):
    from position_induced_transformer_amd import metric
    from test_gpu_mesh_grad import FUSED, LaunchLog
    model = metric.pit_metric(2, 1, 1, 32, 2, 2, orc.grid_mesh_2d(6, False), 0.05, 0.05).cuda()
    assert model._heads_of_block(0, 32) == 0
    mesh = orc.grid_mesh_2d(12, False).cuda()
    log = LaunchLog(monkeypatch)
    model(mesh, torch.randn(2, 144, 1, device="cuda"), mesh).sum().backward()
    assert not [c for c in log.calls if c.startswith(FUSED)], log.calls
    assert log.count("pit_distmat_fwd") == 4 and log.count("pit_distmat_bwd") == 4 and log.count("pit_posatt_fwd_job") == 0


# --------------------------------------------------------------------------- 7. capture
def test_captured_forward_and_backward_replays_on_new_values():
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(31)
    n, b, d = 100, 2, 40
    m = torch.rand(n, n, generator=g).cuda().requires_grad_(True)
    x = torch.randn(b, n, d, generator=g).cuda().requires_grad_(True)
    x2, dy = torch.randn(b, n, d, generator=g).cuda(), torch.randn(b, n, 3 * d, generator=g).cuda()
    c = torch.tensor([11.0, 6.0], device="cuda").requires_grad_(True)
    plan = ops.DistPlan(m, 0.2)

    def step(mm, xx, cc, pl):
        mm.grad = xx.grad = cc.grad = None
        out = ops.posatt_dist_apply(xx, cc, pl, 2, concat=True, head_is_scale=True, m_dist=mm)
        out.backward(dy)
        return out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(m, x, c, plan)                                      # warm-up outside the capture (workspaces)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(m, x, c, plan)
    with torch.no_grad():
        x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    m_e, x_e, c_e = m.detach().clone().requires_grad_(True), x2.clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
    out_e = step(m_e, x_e, c_e, ops.DistPlan(m_e, 0.2))
    assert torch.equal(out, out_e) and torch.equal(x.grad, x_e.grad) and torch.equal(m.grad, m_e.grad)
    assert _err(c.grad, c_e.grad) <= 1e-6                        # (d(scale) meets in fp64 slots: order-free up to the last bits)
