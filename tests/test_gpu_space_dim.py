"""GPU: meshes with 4 to 8 coordinates (space_dim 4..8) against the CPU oracle, which forms the distances with torch.sum over
the last axis as the reference does (pit.py:47,134,190-193,248-253).  The kernels add the squared differences in ATen-CPU's
order, so keep sets match exactly and values to the suite's tolerances: forward 1e-6, gradients 1e-5
of max |ref|.  Such meshes run the per-layer kernels: no fused launch is taken."""
import pytest
import torch

import pit_oracle as orc

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 1e-6, 1e-5
LMDA_TOL = 1e-4                  # d(lmda) against the fp64 oracle, as test_gpu_mesh_grad.py holds it


def _dlmda_fp64(metric, batched, kind, mo, mi, vals, lmda, loc, gout):
    """d(lmda) of the fp64 oracle with the fp32 keep set (a sum over every kept pair: the fp32 oracle's own rounding of it is
    larger than the kernels')."""
    from test_gpu_mesh_grad import fp32_keep_oracle
    lm = lmda.detach().cpu().double().requires_grad_(True)
    with fp32_keep_oracle():
        if kind == "self":
            ref = orc.posatt_self(metric, batched, mi.double(), vals.double(), lm, loc)
        else:
            ref = orc.posatt_cross(metric, batched, mo.double(), mi.double(), vals.double(), lm, loc)
    ref.backward(gout.double())
    return lm.grad
FUSED = ("pit_encoder", "pit_decoder", "pit_block", "pit_fold", "pit_union_att", "pit_posatt_pre", "pit_satt", "pit_slab",
         "pit_edge")


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _lattice(n_per_axis, d):
    """Regular lattice of n_per_axis ** d points in [0, 1]^d: tie shells everywhere, the summation order decides the masks."""
    axes = [torch.linspace(0.0, 1.0, n_per_axis)] * d
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d).contiguous()


class LaunchLog:
    """Names of the library entry points called while active."""

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


def _layer(metric, kind, batched, n_head, dim, loc):
    from position_induced_transformer_amd import pit
    if batched:
        cls = pit.posatt if kind == "self" else pit.posatt_cross
    else:
        cls = {("euclid", "self"): pit.posatt_fixed, ("euclid", "cross"): pit.posatt_cross_fixed,
               ("periodic1d", "self"): pit.posatt_periodic1d, ("periodic1d", "cross"): pit.posatt_cross_periodic1d,
               ("periodic2d", "self"): pit.posatt_periodic2d, ("periodic2d", "cross"): pit.posatt_cross_periodic2d}[(metric, kind)]
    return cls(n_head, dim, loc)


def _meshes(metric, kind, batched, d, b, n_out, n_in, g):
    if metric == "periodic1d":               # uniform spacing along axis 0 (the period comes from it), the rest random
        mi = torch.rand(n_in, d, generator=g)
        mi[:, 0] = torch.arange(n_in, dtype=torch.float32) / n_in
    elif metric == "periodic2d" and d <= 5:  # a lattice (4^4 = 256, 3^5 = 243 points): the period comes from axis 0
        mi = _lattice(4 if d == 4 else 3, d)[:n_in].contiguous()
    elif metric == "periodic2d":
        mi = torch.rand(n_in, d, generator=g)
    else:
        mi = torch.rand((b, n_in, d) if batched else (n_in, d), generator=g)
    if kind == "self":
        return mi, mi
    mo = torch.rand((b, n_out, d) if batched else (n_out, d), generator=g)
    return mo, mi


def _plan(metric, mo, mi, loc, self_attn):
    """The plan the layer builds for these meshes (which kernels run: lists or dense)."""
    from position_induced_transformer_amd import ops
    return ops.MeshPlan(metric, mo.cuda(), mi.cuda(), loc, self_attn)


# locality 0.05 at 240 keys: candidate lists (cap 32, 3 * cap <= n_in); 0.3 at 90 keys: masked dense; 1.0: nothing masked
LAYER_CASES = [
    (d, metric, kind, batched, loc)
    for d in (4, 5, 6, 7, 8)
    for metric, batched in (("euclid", False), ("euclid", True), ("periodic1d", False), ("periodic2d", False))
    for kind in ("self", "cross")
    for loc in (0.05, 0.3, 1.0)
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "d%d-%s-%s-%s-loc%g" % (c[0], c[1], c[2], "b" if c[3] else "f", c[4]))
def test_layer_matches_oracle(case):
    d, metric, kind, batched, loc = case
    g = torch.Generator().manual_seed(1000 + d)
    b, n_head, dim = 3, 2, 8
    n_out, n_in = 70, (240 if loc == 0.05 else 90)
    mo, mi = _meshes(metric, kind, batched, d, b, n_out, n_in, g)
    n_in = mi.shape[-2]
    assert (_plan(metric, mo, mi, loc, kind == "self").nbr_idx is not None) == (loc == 0.05)
    vals = torch.randn(b, n_in, dim, generator=g)
    torch.manual_seed(d)
    layer = _layer(metric, kind, batched, n_head, dim, loc).cuda()
    with torch.no_grad():
        layer.lmda.copy_(torch.randn(n_head, 1, 1, generator=g) * 0.5)
    v = vals.cuda().requires_grad_(True)
    out = layer(mi.cuda(), v) if kind == "self" else layer(mo.cuda(), mi.cuda(), v)
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.cuda())

    lm = layer.lmda.detach().cpu().clone().requires_grad_(True)
    vr = vals.clone().requires_grad_(True)
    if kind == "self":
        ref = orc.posatt_self(metric, batched, mi, vr, lm, loc)
    else:
        ref = orc.posatt_cross(metric, batched, mo, mi, vr, lm, loc)
    ref.backward(gout)
    assert _err(out, ref) <= FWD_TOL
    assert _err(v.grad, vr.grad) <= GRAD_TOL
    assert _err(layer.lmda.grad, _dlmda_fp64(metric, batched, kind, mo, mi, vals, layer.lmda, loc, gout)) <= LMDA_TOL


@pytest.mark.parametrize("d", [4, 5])
def test_lattice_keep_sets_are_exact(d):
    """Tie-heavy lattices: the kept entries of every row are the oracle's exactly."""
    from position_induced_transformer_amd import pit
    mesh = _lattice(4 if d == 4 else 3, d)
    att_mod = pit.posatt_fixed(1, 4, 0.05).cuda()
    with torch.no_grad():
        att_mod.lmda.fill_(0.3)
    att = att_mod.dist2att(mesh.cuda(), mesh.cuda(), att_mod.lmda, 0.05).cpu()
    ref = orc.attention_weights(orc.sqdist("euclid", mesh, mesh), orc.head_scale(att_mod.lmda.detach().cpu()), 0.05, False)
    assert torch.equal(att.reshape(ref.shape) > 0, ref > 0)
    assert _err(att.reshape(ref.shape), ref) <= FWD_TOL


@pytest.mark.parametrize("d,batched", [(6, False), (8, True)])
def test_dist2att_matches_oracle(d, batched):
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(d)
    mo = torch.rand((2, 40, d) if batched else (40, d), generator=g)
    mi = torch.rand((2, 50, d) if batched else (50, d), generator=g)
    mod = (pit.posatt_cross if batched else pit.posatt_cross_fixed)(2, 4, 0.2).cuda()
    att = mod.dist2att(mo.cuda(), mi.cuda(), mod.lmda, 0.2).cpu()
    ref = orc.attention_weights(orc.sqdist("euclid", mo, mi), orc.head_scale(mod.lmda.detach().cpu()), 0.2, batched)
    assert torch.equal(att.reshape(ref.shape) > 0, ref > 0)
    assert _err(att.reshape(ref.shape), ref) <= FWD_TOL


@pytest.mark.parametrize("batched", [False, True])
def test_overflowed_candidate_list(batched):
    """60 duplicated keys overflow the 32-slot candidate lists of the rows next to them: those rows are scanned densely in the
    forward, d(scale) and d(values) (the overflow pass)."""
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(5)
    mi = torch.rand((2, 240, 5) if batched else (240, 5), generator=g)
    mi[..., :60, :] = mi[..., :1, :]
    mo = torch.rand((2, 40, 5) if batched else (40, 5), generator=g)
    mo[..., :10, :] = mi[..., :1, :]
    plan = _plan("euclid", mo, mi, 0.05, False)
    assert plan.nbr_idx is not None and bool((plan.nbr_cnt > plan.nbr_cap).any())
    vals = torch.randn(2, 240, 8, generator=g)
    layer = (pit.posatt_cross if batched else pit.posatt_cross_fixed)(2, 8, 0.05).cuda()
    v = vals.cuda().requires_grad_(True)
    out = layer(mo.cuda(), mi.cuda(), v)
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.cuda())
    lm = layer.lmda.detach().cpu().clone().requires_grad_(True)
    vr = vals.clone().requires_grad_(True)
    ref = orc.posatt_cross("euclid", batched, mo, mi, vr, lm, 0.05)
    ref.backward(gout)
    assert _err(out, ref) <= FWD_TOL
    assert _err(v.grad, vr.grad) <= GRAD_TOL
    assert _err(layer.lmda.grad, _dlmda_fp64("euclid", batched, "cross", mo, mi, vals, layer.lmda, 0.05, gout)) <= LMDA_TOL


def _model_case(kind, d):
    """The task models of the package with d-coordinate meshes: Darcy's fixed-mesh forward on a 4-d lattice, Vorticity's
    periodic one (InstanceNorm after encoder and processor), Elasticity's per-sample point clouds."""
    from position_induced_transformer_amd import tasks
    g = torch.Generator().manual_seed(10 + d)
    torch.manual_seed(10 + d)
    b, in_dim, out_dim, hid, n_head, n_blocks = 2, 1, 1, 16, 2, 2
    norm = False
    if kind in ("fixed", "periodic2d"):
        mesh_in = _lattice(4, d)                                     # 256 points, tie shells
        mesh_ltt = _lattice(3, d)
        mesh_out = mesh_in
        cls = tasks.pit_darcy if kind == "fixed" else tasks.pit_vorticity
        model = cls(d, in_dim, out_dim, hid, n_head, n_blocks, mesh_ltt.cuda(), 0.05, 0.05)
        metric, batched, norm = ("euclid", False, False) if kind == "fixed" else ("periodic2d", False, True)
        func_in = torch.randn(b, mesh_in.shape[0], in_dim, generator=g)
        ref_in = orc.with_coords(mesh_in, func_in)
    else:                                                            # per-sample meshes (Elasticity-like point clouds)
        mesh_in = torch.rand(b, 200, d, generator=g)
        mesh_out = torch.rand(b, 64, d, generator=g)
        mesh_ltt = mesh_out
        model = tasks.pit_elasticity(d, in_dim, out_dim, hid, n_head, n_blocks, None, 0.05, 0.05)
        metric, batched = "euclid", True
        func_in = torch.randn(b, 200, in_dim, generator=g)
        ref_in = func_in
    target = torch.randn(b, mesh_out.shape[-2], out_dim, generator=g)
    return model, metric, batched, n_blocks, norm, mesh_in, func_in, ref_in, mesh_ltt, mesh_out, target


@pytest.mark.parametrize("kind,d", [("fixed", 4), ("batched", 5), ("periodic2d", 4)])
def test_model_forward_loss_backward(kind, d, monkeypatch):
    from position_induced_transformer_amd import utils
    model, metric, batched, n_blocks, norm, mesh_in, func_in, ref_in, mesh_ltt, mesh_out, target = _model_case(kind, d)
    model = model.cuda()
    log = LaunchLog(monkeypatch)
    loss_fn = utils.RelLpNorm(1, 2)
    out = model(mesh_in.cuda(), func_in.cuda(), mesh_out.cuda())
    loss = loss_fn(target.cuda(), out)
    loss.backward()
    torch.cuda.synchronize()
    assert not [c for c in log.calls if c.startswith(FUSED)], sorted(set(log.calls))

    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    ref = orc.pit_apply(p, metric, batched, n_blocks, 0.05, 0.05, mesh_in, ref_in, mesh_ltt, mesh_out, norm)
    ref = ref.reshape(out.shape)
    ref_loss = orc.rel_lp_loss(target, ref, 1, 2)
    ref_loss.backward()
    assert _err(out, ref) <= FWD_TOL * 10                 # (a whole model: the per-layer 1e-6 compounds over five layers)
    assert abs(float(loss) - float(ref_loss)) <= FWD_TOL * 10 * abs(float(ref_loss))
    params = dict(model.named_parameters())
    for k, v in p.items():
        if k in params and params[k].grad is not None:
            tol = LMDA_TOL if k.endswith("lmda") else 2 * GRAD_TOL      # (smoke()'s standard for a whole model's weights)
            assert _err(params[k].grad, v.grad) <= tol, k


def test_captured_train_step_replays_eager():
    from position_induced_transformer_amd.engine import TrainStep
    model, metric, batched, n_blocks, norm, mesh_in, func_in, ref_in, mesh_ltt, mesh_out, target = _model_case("fixed", 4)
    model = model.cuda()
    batch = tuple(t.cuda() for t in (mesh_in, func_in, mesh_out, target))
    eager = TrainStep(model, batch, 1, 2)
    eager.run_eager()
    torch.cuda.synchronize()
    loss_e = float(eager.loss)
    step = TrainStep(model, batch, 1, 2)
    step.capture()
    step.replay()
    torch.cuda.synchronize()
    assert abs(float(step.loss) - loss_e) <= 1e-6 * abs(loss_e)


def test_bf16_mode_layer():
    """The bf16 math mode on the per-layer kernels of a 6-coordinate mesh, at test_gpu_bf16.py's layer tolerance (2e-2 rel-L2)."""
    from position_induced_transformer_amd import ops, pit
    g = torch.Generator().manual_seed(3)
    mi = torch.rand(300, 6, generator=g)
    vals = torch.randn(2, 300, 32, generator=g)
    layer = pit.posatt_fixed(2, 32, 1.0).cuda()
    ops.set_math_mode("bf16")
    try:
        out = layer(mi.cuda(), vals.cuda())
    finally:
        ops.set_math_mode("fp32")
    ref = orc.posatt_self("euclid", False, mi, vals, layer.lmda.detach().cpu(), 1.0)
    rel = float((out.cpu() - ref).norm() / ref.norm())
    assert rel <= 2e-2, rel


def test_space_dim_9_raises_before_any_launch(monkeypatch):
    from position_induced_transformer_amd import pit
    log = LaunchLog(monkeypatch)
    layer = pit.posatt_fixed(2, 4, 0.1).cuda()
    mesh = torch.rand(20, 9, device="cuda")
    with pytest.raises(RuntimeError, match="between 1 and 8"):
        layer(mesh, torch.randn(1, 20, 4, device="cuda"))
    assert not log.calls


@pytest.mark.parametrize("d,loc,n_in", [(4, 0.05, 240), (4, 1.0, 90), (8, 0.05, 240), (8, 0.3, 90)])
def test_mesh_gradients_match_fp64(d, loc, n_in):
    """d(mesh_out) and d(mesh_in) of a cross layer (lists at 0.05, dense otherwise) against the fp64 oracle's autograd, at the
    project's gradient standard; the keep set is the fp32 one (test_gpu_mesh_grad.fp32_keep_oracle)."""
    from test_gpu_mesh_grad import fp32_keep_oracle
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(50 + d)
    mo = torch.rand(60, d, generator=g)
    mi = torch.rand(n_in, d, generator=g)
    assert (_plan("euclid", mo, mi, loc, False).nbr_idx is not None) == (loc == 0.05)
    vals = torch.randn(2, n_in, 8, generator=g)
    layer = pit.posatt_cross_fixed(2, 8, loc).cuda()
    mo_d, mi_d = mo.cuda().requires_grad_(True), mi.cuda().requires_grad_(True)
    out = layer(mo_d, mi_d, vals.cuda())
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.cuda())
    mo_r, mi_r = mo.double().requires_grad_(True), mi.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", False, mo_r, mi_r, vals.double(), layer.lmda.detach().cpu().double(), loc)
    ref.backward(gout.double())
    assert _err(mo_d.grad, mo_r.grad) <= GRAD_TOL
    assert _err(mi_d.grad, mi_r.grad) <= GRAD_TOL


def test_bf16_mode_candidate_list_layer():
    """The bf16 math mode on the candidate-list kernels of a 6-coordinate cross layer, at test_gpu_bf16.py's tolerances."""
    from position_induced_transformer_amd import ops, pit
    g = torch.Generator().manual_seed(4)
    mo, mi = torch.rand(80, 6, generator=g), torch.rand(240, 6, generator=g)
    assert _plan("euclid", mo, mi, 0.05, False).nbr_idx is not None
    vals = torch.randn(2, 240, 32, generator=g)
    layer = pit.posatt_cross_fixed(2, 32, 0.05).cuda()
    v = vals.cuda().requires_grad_(True)
    ops.set_math_mode("bf16")
    try:
        out = layer(mo.cuda(), mi.cuda(), v)
        gout = torch.randn(out.shape, generator=g)
        out.backward(gout.cuda())
    finally:
        ops.set_math_mode("fp32")
    vr = vals.clone().requires_grad_(True)
    ref = orc.posatt_cross("euclid", False, mo, mi, vr, layer.lmda.detach().cpu(), 0.05)
    ref.backward(gout)
    assert float((out.detach().cpu() - ref).norm() / ref.norm()) <= 2e-2
    assert float((v.grad.cpu() - vr.grad).norm() / vr.grad.norm()) <= 5e-2


def test_bf16_mode_model_on_lists():
    """A whole model in the bf16 mode (decoder output and its gradient stored as bf16 on the candidate-list kernels), at
    test_gpu_bf16.py's model tolerances."""
    from position_induced_transformer_amd import ops, utils
    model, metric, batched, n_blocks, norm, mesh_in, func_in, ref_in, mesh_ltt, mesh_out, target = _model_case("fixed", 4)
    model = model.cuda()
    seen = {"bf16_out": 0}
    orig = ops._PosAtt.forward

    def spy(ctx, *a, **k):
        out = orig(ctx, *a, **k)
        if out.dtype == torch.bfloat16:
            seen["bf16_out"] += 1
        return out
    ops._PosAtt.forward = staticmethod(spy)
    ops.set_math_mode("bf16")
    try:
        out = model(mesh_in.cuda(), func_in.cuda(), mesh_out.cuda())
        loss = utils.RelLpNorm(1, 2)(target.cuda(), out)
        loss.backward()
    finally:
        ops.set_math_mode("fp32")
        ops._PosAtt.forward = staticmethod(orig)
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    ref = orc.pit_apply(p, metric, batched, n_blocks, 0.05, 0.05, mesh_in, ref_in, mesh_ltt, mesh_out, norm).reshape(out.shape)
    orc.rel_lp_loss(target, ref, 1, 2).backward()
    assert float((out.detach().cpu() - ref).norm() / ref.norm()) <= 2e-2
    for k, prm in model.named_parameters():
        if prm.grad is not None and not k.endswith("lmda"):
            assert float((prm.grad.cpu() - p[k].grad).norm() / p[k].grad.norm().clamp_min(1e-30)) <= 5e-2, k
    print("bf16 outputs:", seen["bf16_out"])
