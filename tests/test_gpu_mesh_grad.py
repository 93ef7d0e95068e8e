"""GPU: gradients w.r.t. the mesh coordinates (pit.py:47,134 forms the distances with ordinary tensor ops, so the reference's
autograd differentiates through the meshes): pit_posatt_dmesh behind _PosAtt, the per-layer routing of the models, the refusals,
determinism and a few optimiser steps on a mesh parameter - all against the fp64 oracle run through plain autograd.

The oracle keeps the entries that its fp32 twin keeps (the kernels' keep set): a near-tie at the quantile threshold then cannot
flip a mask between precisions and turn a gradient comparison into a comparison of two different functions."""
import contextlib

import pytest
import torch
import torch.nn as nn

import pit_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5                       # max |err| <= TOL * max |ref| per gradient tensor (the project's gradient standard)


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@contextlib.contextmanager
def fp32_keep_oracle():
    """orc.sqdist / orc.attention_weights with the keep set decided in fp32 from the fp32 inputs (the kernels' decision), the
    weights and their gradients in fp64."""
    sq, att = orc.sqdist, orc.attention_weights

    def sqdist(metric, mo, mi):
        m = sq(metric, mo, mi)
        with torch.no_grad():
            m._m32 = sq(metric, mo.detach().float(), mi.detach().float())
        return m

    def attention_weights(m_dist, c, locality, batched):
        with torch.no_grad():
            m32, c32 = getattr(m_dist, "_m32", m_dist.float()), c.detach().float()
            s32 = (m32.unsqueeze(1) * c32) if batched else (m32 * c32)
            keep = s32 <= orc.quantile_threshold(s32, locality)
        scaled = (m_dist.unsqueeze(1) * c) if batched else (m_dist * c)
        scaled = torch.where(keep, scaled, torch.tensor(orc.FLT_MAX, dtype=scaled.dtype, device=scaled.device))
        return torch.softmax(-scaled, dim=-1)

    orc.sqdist, orc.attention_weights = sqdist, attention_weights
    try:
        yield
    finally:
        orc.sqdist, orc.attention_weights = sq, att


class LaunchLog:
    """Names of the library entry points called while active (ops reaches the library through _lib.lib())."""

    def __init__(self, monkeypatch):
        from position_induced_transformer_amd import _lib
        real = _lib.lib()
        self.calls = []
        log = self.calls

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if not callable(fn) or not name.startswith("pit_"):
                    return fn

                def wrapped(*a):
                    log.append(name)
                    return fn(*a)
                return wrapped
        monkeypatch.setattr(_lib, "lib", lambda: Proxy())

    def count(self, name):
        return sum(1 for c in self.calls if c == name)


FUSED = ("pit_encoder", "pit_decoder", "pit_block", "pit_processor", "pit_fold", "pit_union_att", "pit_posatt_pre", "pit_satt",
         "pit_slab", "pit_edge")


def _cloud(b, n, sd, g, batched):
    shape = (b, n, sd) if batched else (n, sd)
    return torch.rand(*shape, generator=g)


# --------------------------------------------------------------------------- 1. the layer matrix
# (kind, heads, space_dim, dim, n_out, n_in, batch, locality)
CASES = [
    ("cross", 1, 2, 44, 100, 150, 3, 1.0),            # dense
    ("cross", 2, 3, 64, 70, 200, 1, 0.05),            # candidate lists
    ("cross", 2, 1, 3, 130, 97, 3, 0.02),
    ("cross", 1, 2, 256, 50, 77, 3, 0.3),              # masked, lists as long as the row: dense masked (cap == 0)
    ("cross_fixed", 2, 2, 44, 90, 130, 3, 0.05),
    ("cross_fixed", 1, 3, 256, 61, 120, 1, 1.0),
    ("cross_fixed", 2, 1, 64, 150, 100, 3, 0.02),
    ("self", 2, 2, 64, 150, 150, 3, 1.0),
    ("self", 1, 3, 3, 130, 130, 1, 0.05),
    ("self_fixed", 1, 2, 44, 97, 97, 3, 1.0),
    ("self_fixed", 2, 3, 256, 200, 200, 3, 0.02),
]


def _module(kind, heads, dim, loc):
    from position_induced_transformer_amd import pit
    cls = {"cross": pit.posatt_cross, "cross_fixed": pit.posatt_cross_fixed, "self": pit.posatt, "self_fixed": pit.posatt_fixed}[kind]
    return cls(heads, dim, loc).cuda()


def _run_layer(mod, kind, mo, mi, x, dy, mesh_grad):
    mo = mo.cuda().requires_grad_(mesh_grad)
    mi = mo if kind.startswith("self") else mi.cuda().requires_grad_(mesh_grad)
    xv = x.cuda().requires_grad_(True)
    mod.lmda.grad = None
    out = mod(mo, xv) if kind.startswith("self") else mod(mo, mi, xv)
    out.backward(dy.cuda())
    return out, mo.grad, (None if mi is mo else mi.grad), xv.grad, mod.lmda.grad.clone()


def _oracle_layer(mod, kind, mo, mi, x, dy, batched):
    lm = mod.lmda.detach().double().cpu().requires_grad_(True)
    mo64 = mo.double().requires_grad_(True)
    mi64 = mo64 if kind.startswith("self") else mi.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    with fp32_keep_oracle():
        if kind.startswith("self"):
            out = orc.posatt_self("euclid", batched, mo64, x64, lm, mod.locality)
        else:
            out = orc.posatt_cross("euclid", batched, mo64, mi64, x64, lm, mod.locality)
    out.backward(dy.double())
    return out, mo64.grad, (None if mi64 is mo64 else mi64.grad), x64.grad, lm.grad


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-h{c[1]}-s{c[2]}-d{c[3]}-{c[4]}x{c[5]}-b{c[6]}-loc{c[7]}" for c in CASES])
def test_layer_mesh_gradients_match_fp64(case):
    kind, heads, sd, dim, n_out, n_in, b, loc = case
    batched = not kind.endswith("fixed")
    if kind.startswith("self"):
        n_in = n_out
    g = torch.Generator().manual_seed(CASES.index(case))
    torch.manual_seed(1)
    mod = _module(kind, heads, dim, loc)
    mo, mi = _cloud(b, n_out, sd, g, batched), _cloud(b, n_in, sd, g, batched)
    x = torch.randn(b, n_in, dim, generator=g)
    width = (heads + 1) * dim if kind.startswith("self") else heads * dim
    dy = torch.randn(b, n_out, width, generator=g)
    got = _run_layer(mod, kind, mo, mi, x, dy, True)
    ref = _oracle_layer(mod, kind, mo, mi, x, dy, batched)
    errs = {"out": _err(got[0], ref[0]), "d_mesh_out": _err(got[1], ref[1]), "d_values": _err(got[3], ref[3]),
            "d_lmda": _err(got[4].reshape(-1), ref[4].reshape(-1))}
    if ref[2] is not None:
        errs["d_mesh_in"] = _err(got[2], ref[2])
    print(case, errs)
    assert max(errs.values()) <= TOL, errs
    # values / lmda gradients do not depend on whether the meshes require grad
    plain = _run_layer(mod, kind, mo, mi, x, dy, False)
    assert plain[1] is None and plain[2] is None
    assert float((plain[3] - got[3]).norm() / plain[3].norm()) <= 1e-6
    assert float((plain[4] - got[4]).norm() / plain[4].norm()) <= 1e-6


def test_overflowed_candidate_lists_mesh_gradients_match_fp64():
    """Coincident key points (tie shells beyond the list capacity): the overflowed rows are scanned densely in both passes."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(11)
    mo, mi = torch.rand(2, 150, 2, generator=g), torch.rand(2, 160, 2, generator=g)
    mi[:, 40:120] = mi[:, 40:41]
    x, c = torch.randn(2, 160, 32, generator=g), torch.tensor([14.0, 9.0])
    dy = torch.randn(2, 150, 64, generator=g)
    mo1, mi1, x1 = mo.cuda().requires_grad_(True), mi.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    plan = ops.MeshPlan("euclid", mo1, mi1, 0.1, False)
    assert plan.nbr_idx is not None and bool((plan.nbr_cnt > plan.nbr_cap).any())
    out = ops.posatt_apply(x1, c.cuda(), plan, 2, concat=False, head_is_scale=True, mesh_out=mo1, mesh_in=mi1)
    out.backward(dy.cuda())
    mo64, mi64, x64 = mo.double().requires_grad_(True), mi.double().requires_grad_(True), x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", True, mo64, mi64, x64, None, 0.1, c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    errs = [_err(mo1.grad, mo64.grad), _err(mi1.grad, mi64.grad), _err(x1.grad, x64.grad)]
    print("overflow", errs)
    assert max(errs) <= TOL, errs


# --------------------------------------------------------------------------- 2. models
def _params64(model):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters() if k != "mesh_ltt"}


# d(lmda) is one scalar per head, formed by the existing d(scale) kernels as a sum over every (row, key, channel) term, and those
# terms cancel: measured 2.2e-5 of |ref| for NACA's up.lmda (1 head, 11271 x 196 weights), everything else <= 1e-6.  That error is
# the fp32 forming of the terms, not the mesh-gradient path, so the lmda scalars are held to 1e-4 here.
LMDA_TOL = 1e-4


def _check_params(model, p64, errs):
    for k, v in model.named_parameters():
        if k in p64:
            errs[("d_" + k) if not k.endswith("lmda") else ("lmda:d_" + k)] = _err(v.grad, p64[k].grad)


def _assert_errs(errs):
    worst = max(v for k, v in errs.items() if not k.startswith("lmda:"))
    worst_l = max([v for k, v in errs.items() if k.startswith("lmda:")] or [0.0])
    assert worst <= TOL and worst_l <= LMDA_TOL, errs


def test_elasticity_mesh_gradients_match_fp64():
    """Per-sample cloud, latent mesh = output mesh: the encoder's row terms, the processor's self terms and the decoder's key
    terms all land on mesh_out."""
    from position_induced_transformer_amd import tasks
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(3)
    model = tasks.pit_elasticity(2, 5, 1, 32, 2, 2, None, 0.05, 0.05).cuda()
    xy = torch.rand(2, 150, 2, generator=g)
    mi, mo = xy.clone(), (xy + 0.01 * torch.rand(2, 150, 2, generator=g))
    f = torch.randn(2, 150, 5, generator=g)
    dy = torch.randn(2, 150, 1, generator=g)
    mi1, mo1 = mi.cuda().requires_grad_(True), mo.cuda().requires_grad_(True)
    model(mi1, f.cuda(), mo1).backward(dy.cuda())
    p64 = _params64(model)
    mi64, mo64 = mi.double().requires_grad_(True), mo.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.pit_apply(p64, "euclid", True, 2, 0.05, 0.05, mi64, f.double(), mo64, mo64)
    ref.backward(dy.double())
    errs = {"d_mesh_in": _err(mi1.grad, mi64.grad), "d_mesh_out": _err(mo1.grad, mo64.grad)}
    _check_params(model, p64, errs)
    print("elasticity", errs)
    _assert_errs(errs)


def test_naca_mesh_gradients_match_fp64():
    """Latent mesh = a strided view of mesh_out: its gradient flows back through the view onto the grid."""
    from position_induced_transformer_amd import tasks
    torch.manual_seed(4)
    g = torch.Generator().manual_seed(4)
    model = tasks.pit_naca(2, 2, 4, 32, 1, 2, None, 8, 8, 0.05, 0.05).cuda()
    b = 2
    outline = torch.rand(b, 60, 2, generator=g)
    grid = torch.rand(b, 221, 51, 2, generator=g)
    dy = torch.randn(b, 221, 51, 4, generator=g)
    mi1, grid1 = outline.cuda().requires_grad_(True), grid.cuda().requires_grad_(True)
    model(mi1, outline.cuda(), grid1).backward(dy.cuda())
    p64 = _params64(model)
    mi64, grid64 = outline.double().requires_grad_(True), grid.double().requires_grad_(True)
    ltt = grid64[:, ::8, ::8, :][:, :model.x_res, :model.y_res, :].reshape(b, -1, 2)
    with fp32_keep_oracle():
        ref = orc.pit_apply(p64, "euclid", True, 2, 0.05, 0.05, mi64, outline.double(), ltt, grid64.reshape(b, -1, 2))
    ref.reshape(dy.shape).backward(dy.double())
    errs = {"d_mesh_in": _err(mi1.grad, mi64.grad), "d_mesh_out": _err(grid1.grad, grid64.grad)}
    _check_params(model, p64, errs)
    print("naca", errs)
    _assert_errs(errs)


def _darcy(seed=5):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    ltt = tasks.grid_mesh_2d(8, True)
    model = tasks.pit_darcy(2, 1, 1, 32, 2, 2, ltt, 0.05, 0.05).cuda()
    model.mesh_ltt = nn.Parameter(model.mesh_ltt.detach().clone().cuda())
    return model


def _darcy_oracle(model, p64, ltt64, mesh64, f, mesh_out64=None):
    mesh_out64 = mesh64 if mesh_out64 is None else mesh_out64
    flat_in = mesh64.reshape(-1, 2)
    with fp32_keep_oracle():
        return orc.pit_apply(p64, "euclid", False, 2, 0.05, 0.05, flat_in, orc.with_coords(flat_in, f.double().reshape(f.shape[0], -1, 1)),
                             ltt64, mesh_out64.reshape(-1, 2))


def test_darcy_mesh_and_latent_mesh_gradients_match_fp64():
    """Batch-free meshes summed over the batch; mesh_in also feeds the coordinate channels of the encoder input."""
    from position_induced_transformer_amd import tasks
    model = _darcy()
    g = torch.Generator().manual_seed(5)
    mesh_in = tasks.grid_mesh_2d(20, True) + 0.01 * torch.rand(20, 20, 2, generator=g)
    mesh_out = tasks.grid_mesh_2d(20, True) + 0.01 * torch.rand(20, 20, 2, generator=g)
    f = torch.randn(3, 20, 20, 1, generator=g)
    dy = torch.randn(3, 20, 20, 1, generator=g)
    mi1, mo1 = mesh_in.cuda().requires_grad_(True), mesh_out.cuda().requires_grad_(True)
    model(mi1, f.cuda(), mo1).backward(dy.cuda())
    p64 = _params64(model)
    ltt64 = model.mesh_ltt.detach().double().cpu().requires_grad_(True)
    mi64, mo64 = mesh_in.double().requires_grad_(True), mesh_out.double().requires_grad_(True)
    ref = _darcy_oracle(model, p64, ltt64, mi64, f, mo64)
    ref.reshape(dy.shape).backward(dy.double())
    errs = {"d_mesh_in": _err(mi1.grad, mi64.grad), "d_mesh_out": _err(mo1.grad, mo64.grad),
            "d_mesh_ltt": _err(model.mesh_ltt.grad, ltt64.grad)}
    _check_params(model, p64, errs)
    print("darcy", errs)
    _assert_errs(errs)


# --------------------------------------------------------------------------- 3. spies
def test_mesh_gradient_path_runs_one_dmesh_per_layer_and_no_fused_launch(monkeypatch):
    from position_induced_transformer_amd import tasks
    model = _darcy()
    mesh = tasks.grid_mesh_2d(20, True).cuda()
    f = torch.randn(3, 20, 20, 1, device="cuda")
    log = LaunchLog(monkeypatch)
    mesh_g = mesh.clone().requires_grad_(True)
    model(mesh_g, f, mesh_g).sum().backward()
    n_att = 2 + len(model.conv)
    assert log.count("pit_posatt_dmesh") == n_att, log.calls
    assert not [c for c in log.calls if c.startswith(FUSED)], log.calls
    log.calls.clear()
    model.mesh_ltt.requires_grad_(False)
    model(mesh, f, mesh).sum().backward()
    assert log.count("pit_posatt_dmesh") == 0
    with torch.no_grad():
        model(mesh_g, f, mesh_g)
    assert log.count("pit_posatt_dmesh") == 0


# --------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("name", ["burgers", "vorticity"])
def test_periodic_models_refuse_mesh_gradients_before_any_launch(name, monkeypatch):
    from position_induced_transformer_amd import tasks
    model, sample, _meta = tasks.make_task(name)
    mesh_in, func_in, mesh_out, _y = sample(2)
    log = LaunchLog(monkeypatch)
    with pytest.raises(NotImplementedError, match="period"):
        model(mesh_in.clone().requires_grad_(True), func_in, mesh_out)
    assert log.calls == []
    with torch.no_grad():
        out = model(mesh_in.clone().requires_grad_(True), func_in, mesh_out)
    assert torch.isfinite(out).all()


def test_bf16_mode_refuses_mesh_gradients_before_any_launch(monkeypatch):
    from position_induced_transformer_amd import ops
    model = _darcy()
    mesh = torch.rand(20 * 20, 2, device="cuda")
    f = torch.randn(2, 400, 1, device="cuda")
    with ops.math_mode("bf16"):
        log = LaunchLog(monkeypatch)
        with pytest.raises(NotImplementedError, match="fp32"):
            model(mesh, f, mesh)                       # the latent mesh parameter requires grad
        assert log.calls == []
        with torch.no_grad():
            assert torch.isfinite(model(mesh, f, mesh)).all()


# --------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("kind", ["dense", "dense-fixed", "lists", "lists-fixed", "overflow", "self-dense"])
def test_mesh_gradients_are_the_same_bits_on_every_run(kind):
    """pit_posatt_dmesh sums its per-sample partials in a fixed order (no atomics): the same d_out gives the same bits.  (Through a
    whole model the d_out a layer receives may itself differ in the last bits from run to run: the MLP backward kernels add some
    partial sums with atomics - that is upstream of this op.)"""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(12)
    batched = not kind.endswith("fixed")
    n_out, n_in = (120, 120) if kind == "self-dense" else (150, 160)
    mo = _cloud(3, n_out, 2, g, batched)
    mi = mo if kind == "self-dense" else _cloud(3, n_in, 2, g, batched)
    if kind == "overflow":
        mi[:, 40:120] = mi[:, 40:41]
    loc = 1.0 if "dense" in kind else 0.1
    x = torch.randn(3, n_in, 48, generator=g).cuda()
    concat = kind == "self-dense"
    dy = torch.randn(3, n_out, (3 if concat else 2) * 48, generator=g).cuda()
    c = torch.tensor([14.0, 9.0], device="cuda")
    grads = []
    for _ in range(2):
        mo1 = mo.cuda().requires_grad_(True)
        mi1 = mo1 if concat else mi.cuda().requires_grad_(True)
        plan = ops.MeshPlan("euclid", mo1, mi1, loc, concat)
        assert (plan.nbr_idx is not None) == (loc < 1.0)
        out = ops.posatt_apply(x, c, plan, 2, concat=concat, head_is_scale=True, mesh_out=mo1, mesh_in=mi1)
        out.backward(dy)
        grads.append((mo1.grad.clone(), mi1.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


# --------------------------------------------------------------------------- 6. shape optimisation
def test_adam_on_the_latent_mesh_follows_fp64_and_rebuilds_the_plans():
    from position_induced_transformer_amd import tasks
    model = _darcy()
    mesh = tasks.grid_mesh_2d(20, True)
    f = torch.randn(2, 20, 20, 1, generator=torch.Generator().manual_seed(7))
    p64 = _params64(model)
    ltt64 = model.mesh_ltt.detach().double().cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([model.mesh_ltt], lr=1e-3, eps=1e-3)
    opt64 = torch.optim.Adam([ltt64], lr=1e-3, eps=1e-3)
    keys = set()
    for _step in range(3):
        opt.zero_grad()
        model(mesh.cuda(), f.cuda(), mesh.cuda()).square().sum().backward()
        keys |= set(model.conv[0]._plans)
        opt.step()
        opt64.zero_grad()
        _darcy_oracle(model, p64, ltt64, mesh.double(), f).square().sum().backward()
        opt64.step()
        err = float((model.mesh_ltt.detach().double().cpu() - ltt64.detach()).abs().max())
        print("adam darcy step", _step, err)
        assert err <= 1e-5
    assert len(keys) == 3                  # a new plan for every version of the latent mesh


def test_adam_on_a_per_sample_mesh_follows_fp64():
    from position_induced_transformer_amd import tasks
    torch.manual_seed(8)
    model = tasks.pit_elasticity(2, 5, 1, 32, 2, 2, None, 0.05, 0.05).cuda()
    g = torch.Generator().manual_seed(8)
    xy = torch.rand(2, 150, 2, generator=g)
    f = torch.randn(2, 150, 5, generator=g)
    mesh = nn.Parameter(xy.cuda())
    mesh64 = xy.double().clone().requires_grad_(True)
    p64 = _params64(model)
    opt, opt64 = torch.optim.Adam([mesh], lr=1e-3, eps=1e-3), torch.optim.Adam([mesh64], lr=1e-3, eps=1e-3)
    for _step in range(3):
        opt.zero_grad()
        model(mesh, f.cuda(), mesh).square().sum().backward()
        opt.step()
        opt64.zero_grad()
        with fp32_keep_oracle():
            orc.pit_apply(p64, "euclid", True, 2, 0.05, 0.05, mesh64, f.double(), mesh64, mesh64).square().sum().backward()
        opt64.step()
        err = float((mesh.detach().double().cpu() - mesh64.detach()).abs().max())
        print("adam elasticity step", _step, err)
        assert err <= 1e-5


# --------------------------------------------------------------------------- 7. dist2att
@pytest.mark.parametrize("batched", [True, False])
def test_dist2att_is_differentiable_in_both_meshes(batched):
    from position_induced_transformer_amd import pit
    torch.manual_seed(9)
    g = torch.Generator().manual_seed(9)
    mod = (pit.posatt_cross if batched else pit.posatt_cross_fixed)(2, 8, 0.1).cuda()
    mo, mi = _cloud(2, 40, 2, g, batched), _cloud(2, 70, 2, g, batched)
    w = torch.randn(*((2, 2, 40, 70) if batched else (2, 40, 70)), generator=g)
    mo1, mi1 = mo.cuda().requires_grad_(True), mi.cuda().requires_grad_(True)
    (mod.dist2att(mo1, mi1, mod.lmda, mod.locality) * w.cuda()).sum().backward()
    mo64, mi64 = mo.double().requires_grad_(True), mi.double().requires_grad_(True)
    with fp32_keep_oracle():
        att = orc.attention_weights(orc.sqdist("euclid", mo64, mi64), orc.head_scale(mod.lmda.detach().double().cpu()), 0.1, batched)
    (att * w.double()).sum().backward()
    errs = [_err(mo1.grad, mo64.grad), _err(mi1.grad, mi64.grad)]
    print("dist2att", errs)
    assert max(errs) <= TOL, errs
