"""The reproducible mode (ops.set_reproducible) on the GPU: the ordered MFMA weight-gradient contraction
against fp64 and bit for bit across runs, the sorted transposed lists and the ordered overflow pass, whole models."""
import types

import pytest
import torch

import pit_oracle as orc
from test_gpu_mesh_grad import FUSED, LaunchLog, fp32_keep_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5                       # max |err| <= TOL * max |ref| per gradient tensor (the project's gradient standard)


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def _noise():
    """Unrelated device work between two runs: a large GEMM (other workgroups in flight, other arrival orders)."""
    a = torch.randn(2048, 2048, device="cuda")
    return (a @ a).sum()


# --------------------------------------------------------------------------- 1. the contraction, raw ABI
SHAPES = [(r, *n) for n in [(3, 32, 32), (192, 64, 64), (44, 128, 1), (384, 128, 128)] for r in (1, 63, 64, 65, 257, 1000, 4099)]
SHAPES.append((300, 768, 256, 256))


def _dw_call(x, h, d_y, scratch, out_gelu, acc, n0, n1, n2, grads):
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    rows = x.shape[0]
    nbytes = int(L.pit_mlp_bwd_params_ordered_mfma_workspace(rows, n0, n1, n2))
    assert nbytes > 0
    work = torch.full((nbytes // 4,), float("nan"), device="cuda")
    g = [t.clone() for t in grads]
    rc = L.pit_mlp_bwd_params_ordered_mfma(x.data_ptr(), x.stride(0), rows, n0, n1, n2, h.data_ptr(), out_gelu, d_y.data_ptr(),
                                           d_y.stride(0), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), acc,
                                           scratch.data_ptr(), work.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "pit_mlp_bwd_params_ordered_mfma")
    return g


@pytest.mark.parametrize("shape", SHAPES, ids=[f"r{s[0]}-{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
@pytest.mark.parametrize("out_gelu,acc,pad", [(0, 0, 0), (1, 1, 0), (0, 1, 5), (1, 0, 5)])
def test_ordered_mfma_contraction_matches_fp64_and_repeats_bit_for_bit(shape, out_gelu, acc, pad):
    rows, n0, n1, n2 = shape
    g = torch.Generator().manual_seed(rows * 7 + n0 + out_gelu + 2 * acc)
    xs = torch.randn(rows, n0 + pad, generator=g).cuda()
    dys = torch.randn(rows, n2 + pad, generator=g).cuda()
    x, d_y = xs[:, :n0], dys[:, :n2]                       # ldx / ld_dy larger than the width when pad > 0
    h = torch.randn(rows, n1, generator=g).cuda()
    scratch = torch.randn(rows * (n1 + n2), generator=g).cuda()       # dZ1 | dZ2 in the layout of pit_mlp_bwd_data
    dz1 = scratch[:rows * n1].view(rows, n1)
    dz2 = scratch[rows * n1:].view(rows, n2) if out_gelu else d_y
    grads = [torch.randn(s, generator=g).cuda() for s in [(n1, n0), (n1,), (n2, n1), (n2,)]]
    ref = [dz1.double().t() @ x.double(), dz1.double().sum(0), dz2.double().t() @ h.double(), dz2.double().sum(0)]
    if acc:
        ref = [r + g0.double() for r, g0 in zip(ref, grads)]
    runs = []
    for i in range(3):
        runs.append(_dw_call(x, h, d_y, scratch, out_gelu, acc, n0, n1, n2, grads))
        _noise()
    # the same operands at other addresses
    xs2, dys2, h2, sc2 = (torch.cat((torch.zeros(64, device="cuda"), t.reshape(-1))) [64:].view(t.shape) for t in (xs, dys, h, scratch))
    runs.append(_dw_call(xs2[:, :n0], h2, dys2[:, :n2], sc2, out_gelu, acc, n0, n1, n2, grads))
    torch.cuda.synchronize()
    errs = [_err(a, b) for a, b in zip(runs[0], ref)]
    print(shape, out_gelu, acc, pad, errs)
    assert max(errs) <= TOL, errs
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# --------------------------------------------------------------------------- 2. the list kernels
def _ranges_sorted(plan, srt):
    ptr, raw, srt = plan.rev_ptr.cpu(), plan.rev_row.cpu(), srt.cpu()
    n = 0
    for mb in range(ptr.shape[0]):
        for j in range(ptr.shape[1] - 1):
            a, b = int(ptr[mb, j]), int(ptr[mb, j + 1])
            if b - a < 1:
                continue
            got, was = srt[mb, a:b], raw[mb, a:b]
            real = got[got >= 0]
            assert bool((real[1:] > real[:-1]).all()), (mb, j, got)
            assert bool((got[len(real):] == -1).all())
            assert torch.equal(torch.sort(got).values, torch.sort(was).values)
            n += 1
    assert n > 0


def test_sorted_reverse_lists_are_ascending_permutations(monkeypatch):
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(11)
    mo, mi = torch.rand(2, 150, 2, generator=g).cuda(), torch.rand(2, 160, 2, generator=g).cuda()
    log = LaunchLog(monkeypatch)
    with ops.reproducible():
        per_sample = ops.MeshPlan("euclid", mo, mi, 0.1, False)
        fixed = ops.MeshPlan("euclid", mo[0], mi[0], 0.1, False)
        for plan in (per_sample, fixed):
            assert plan.nbr_idx is not None
            plan.ensure_reverse_lists()
            srt = plan.sorted_reverse_lists()
            assert srt is plan.sorted_reverse_lists()                  # (the plan carries it)
            _ranges_sorted(plan, srt)
    assert log.count("pit_lists_sort_ranges") == 2, log.calls


def test_key_range_beyond_the_lds_sort_is_sorted_too():
    """Raw ABI: 5000 rows of capacity 2 all list key 3 (a range of 5000 entries, beyond the 4096 the LDS sort holds: the rank
    sort) and one of eight other keys (ranges of ~600: the LDS sort); every 97th row overflowed (its slots stay -1)."""
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    n_out, n_in, cap = 5000, 16, 2
    rows = torch.arange(n_out)
    idx = torch.stack((torch.full((n_out,), 3), 4 + rows.flip(0) % 8), 1).int().cuda().contiguous()
    cnt = torch.where(rows % 97 == 0, cap + 1, cap).int().cuda()
    ptr = torch.empty((1, n_in + 1), dtype=torch.int32, device="cuda")
    raw = torch.empty((1, n_out * cap), dtype=torch.int32, device="cuda")
    work = torch.empty((2 * n_in,), dtype=torch.int32, device="cuda")
    _lib.check(L.pit_lists_transpose(idx.data_ptr(), cnt.data_ptr(), 1, n_out, n_in, cap, ptr.data_ptr(), raw.data_ptr(),
                                     work.data_ptr(), _lib.stream_ptr()), "pit_lists_transpose")
    srt = raw.clone()
    _lib.check(L.pit_lists_sort_ranges(ptr.data_ptr(), raw.data_ptr(), 1, n_in, n_out * cap, srt.data_ptr(), _lib.stream_ptr()),
               "pit_lists_sort_ranges")
    torch.cuda.synchronize()
    assert int(ptr[0, 4] - ptr[0, 3]) == n_out > 4096
    _ranges_sorted(types.SimpleNamespace(rev_ptr=ptr, rev_row=raw), srt)
    key3 = srt[0, int(ptr[0, 3]):int(ptr[0, 4])].cpu()
    listed = rows[rows % 97 != 0].int()
    assert torch.equal(key3[:len(listed)], listed) and bool((key3[len(listed):] == -1).all())


def _overflow_case():
    g = torch.Generator().manual_seed(11)
    mo, mi = torch.rand(2, 150, 2, generator=g), torch.rand(2, 160, 2, generator=g)
    mi[:, 40:120] = mi[:, 40:41]
    x, c = torch.randn(2, 160, 32, generator=g), torch.tensor([14.0, 9.0])
    dy = torch.randn(2, 150, 64, generator=g)
    return mo, mi, x, c, dy


def test_overflowed_rows_reach_d_values_in_a_fixed_order(monkeypatch):
    from position_induced_transformer_amd import ops
    mo, mi, x, c, dy = _overflow_case()
    x64 = x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", True, mo.double(), mi.double(), x64, None, 0.1, c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    log = LaunchLog(monkeypatch)
    runs = []
    with ops.reproducible():
        for _ in range(3):
            plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), 0.1, False)          # a fresh plan: a fresh transpose
            assert plan.nbr_idx is not None and bool((plan.nbr_cnt > plan.nbr_cap).any())
            x1 = x.cuda().requires_grad_(True)
            out = ops.posatt_apply(x1, c.cuda(), plan, 2, concat=False, head_is_scale=True)
            out.backward(dy.cuda())
            runs.append(x1.grad.clone())
            _noise()
    torch.cuda.synchronize()
    err = _err(runs[0], x64.grad)
    print("overflow d_values", err)
    assert err <= TOL
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert log.count("pit_posatt_overflow_dv_ordered") == 3 and log.count("pit_lists_sort_ranges") == 3, log.calls


def _three_runs(build):
    """build() -> (d_values of a fresh plan and layer run, the plan): three runs with unrelated work in between."""
    from position_induced_transformer_amd import ops
    runs = []
    with ops.reproducible():
        for _ in range(3):
            grad, plan = build()
            assert plan.nbr_idx is not None and bool((plan.nbr_cnt > plan.nbr_cap).any())      # rows really overflowed
            runs.append(grad.clone())
            _noise()
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    return runs[0]


@pytest.mark.parametrize("sd", [4, 5, 8])
def test_overflowed_rows_on_meshes_of_4_to_8_coordinates(sd, monkeypatch):
    """4 coordinates and beyond take the 8-coordinate instance, like every list kernel: all coordinates enter the distance."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(20 + sd)
    mo, mi = torch.rand(2, 150, sd, generator=g), torch.rand(2, 160, sd, generator=g)
    mi[:, 40:120] = mi[:, 40:41]
    x, c, dy = torch.randn(2, 160, 32, generator=g), torch.tensor([14.0, 9.0]), torch.randn(2, 150, 64, generator=g)
    x64 = x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", True, mo.double(), mi.double(), x64, None, 0.1, c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    log = LaunchLog(monkeypatch)

    def build():
        plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), 0.1, False)
        x1 = x.cuda().requires_grad_(True)
        ops.posatt_apply(x1, c.cuda(), plan, 2, concat=False, head_is_scale=True).backward(dy.cuda())
        return x1.grad, plan
    err = _err(_three_runs(build), x64.grad)
    print("overflow d_values, space_dim", sd, err)
    assert err <= TOL
    assert log.count("pit_posatt_overflow_dv_ordered") == 3, log.calls


def test_overflowed_rows_on_a_mesh_shared_by_the_batch(monkeypatch):
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(31)
    mo, mi = torch.rand(150, 2, generator=g), torch.rand(160, 2, generator=g)
    mi[40:120] = mi[40:41]
    x, c, dy = torch.randn(3, 160, 32, generator=g), torch.tensor([14.0, 9.0]), torch.randn(3, 150, 64, generator=g)
    x64 = x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", False, mo.double(), mi.double(), x64, None, 0.1, c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    log = LaunchLog(monkeypatch)

    def build():
        plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), 0.1, False)
        x1 = x.cuda().requires_grad_(True)
        ops.posatt_apply(x1, c.cuda(), plan, 2, concat=False, head_is_scale=True).backward(dy.cuda())
        return x1.grad, plan
    err = _err(_three_runs(build), x64.grad)
    print("overflow d_values, fixed mesh", err)
    assert err <= TOL
    assert log.count("pit_posatt_overflow_dv_ordered") == 3, log.calls


def test_overflowed_rows_with_coordinate_channels_read_from_the_mesh(monkeypatch):
    """coord_dims = 2 (the Darcy encoder's tagged input): the coordinate channels get no gradient, the others shift by two."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(32)
    mo, mi = torch.rand(150, 2, generator=g), torch.rand(160, 2, generator=g)
    mi[40:120] = mi[40:41]
    f, c, dy = torch.randn(3, 160, 6, generator=g), torch.tensor([14.0, 9.0]), torch.randn(3, 150, 16, generator=g)
    f64 = f.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", False, mo.double(), mi.double(), orc.with_coords(mi.double(), f64), None, 0.1,
                               c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    log = LaunchLog(monkeypatch)

    def build():
        plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), 0.1, False)
        f1 = f.cuda().requires_grad_(True)
        ops.posatt_apply(f1, c.cuda(), plan, 2, concat=False, head_is_scale=True, coord_dims=2).backward(dy.cuda())
        return f1.grad, plan
    err = _err(_three_runs(build), f64.grad)
    print("overflow d_values, coord_dims 2", err)
    assert err <= TOL
    assert log.count("pit_posatt_overflow_dv_ordered") == 3, log.calls


def test_overflowed_rows_of_a_self_attention_layer_with_concat(monkeypatch):
    """concat: the attention output starts at column d of d_out (out_col0 = d)."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(33)
    m = torch.rand(2, 150, 2, generator=g)
    m[:, 40:120] = m[:, 40:41]
    x, c, dy = torch.randn(2, 150, 32, generator=g), torch.tensor([14.0, 9.0]), torch.randn(2, 150, 96, generator=g)
    x64 = x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_self("euclid", True, m.double(), x64, None, 0.1, c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    log = LaunchLog(monkeypatch)

    def build():
        mc = m.cuda()
        plan = ops.MeshPlan("euclid", mc, mc, 0.1, True)
        x1 = x.cuda().requires_grad_(True)
        ops.posatt_apply(x1, c.cuda(), plan, 2, concat=True, head_is_scale=True).backward(dy.cuda())
        return x1.grad, plan
    err = _err(_three_runs(build), x64.grad)
    print("overflow d_values, concat", err)
    assert err <= TOL
    assert log.count("pit_posatt_overflow_dv_ordered") == 3, log.calls


def test_union_kind_plan_takes_d_values_from_the_sorted_lists(monkeypatch):
    """A NACA-like layer below 2 k rows: per-sample body-fitted (jittered) grids, 2 x 32^2 rows on 2 x 16^2 keys - the plan takes
    the union-tile forward; in the mode d(values) comes from the sorted lists, not from the union tiles' atomic adds."""
    from position_induced_transformer_amd import ops, tasks
    g = torch.Generator().manual_seed(41)
    mo = (tasks.grid_mesh_2d(32, True).reshape(1, -1, 2) + 0.004 * torch.rand(2, 1024, 2, generator=g))
    mi = (tasks.grid_mesh_2d(16, True).reshape(1, -1, 2) + 0.008 * torch.rand(2, 256, 2, generator=g))
    x, c, dy = torch.randn(2, 256, 32, generator=g), torch.tensor([14.0, 9.0]), torch.randn(2, 1024, 64, generator=g)
    x64 = x.double().requires_grad_(True)
    with fp32_keep_oracle():
        ref = orc.posatt_cross("euclid", True, mo.double(), mi.double(), x64, None, 0.05, c=c.double().reshape(2, 1, 1))
    ref.backward(dy.double())
    log = LaunchLog(monkeypatch)
    runs = []
    with ops.reproducible():
        for _ in range(3):
            plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), 0.05, False)
            assert plan.nbr_idx is not None and plan.union_tiles()
            x1 = x.cuda().requires_grad_(True)
            ops.posatt_apply(x1, c.cuda(), plan, 2, concat=False, head_is_scale=True).backward(dy.cuda())
            runs.append(x1.grad.clone())
            _noise()
    torch.cuda.synchronize()
    err = _err(runs[0], x64.grad)
    print("union-kind d_values", err)
    assert err <= TOL
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert log.count("pit_lists_sort_ranges") == 3, log.calls


# --------------------------------------------------------------------------- 3. the loss, raw ABI
@pytest.mark.parametrize("b,npts,nch,p", [(3, 150, 2, 2), (5, 1849, 1, 1), (2, 20000, 1, 2), (4100, 7, 1, 2)],
                         ids=["one-workgroup", "one-workgroup-p1", "series-too-long", "too-many-pairs"])
def test_ordered_loss_matches_fp64_and_repeats_bit_for_bit(b, npts, nch, p):
    """pit_rel_lp_loss_fwd_grad_ordered: the one-workgroup-per-series kernel, and beyond its envelope (more than 16384 points, more
    than 4096 pairs) the 256-thread kernel with the series not split.  fp32 inputs, fp64 sums: 1e-6 of the reference (norms,
    loss), gradients to the project's 1e-5; the workspace is left zero; three calls give the same bits."""
    from position_induced_transformer_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(b + npts)
    t, q = torch.randn(b, npts, nch, generator=g).cuda(), torch.randn(b, npts, nch, generator=g).cuda()
    ws = torch.zeros(4 + 5 * b * nch, device="cuda")
    q64 = q.double().cpu().requires_grad_(True)
    ref = orc.rel_lp_loss(t.double().cpu(), q64, nch, p)
    ref.backward()
    runs = []
    for _ in range(3):
        norms, loss, dq = torch.empty(b, nch, 2, device="cuda"), torch.empty((), device="cuda"), torch.empty_like(q)
        rc = L.pit_rel_lp_loss_fwd_grad_ordered(t.data_ptr(), q.data_ptr(), None, None, b, npts, nch, p, norms.data_ptr(),
                                                loss.data_ptr(), ws.data_ptr(), dq.data_ptr(), None, None, 0, _lib.stream_ptr())
        _lib.check(rc, "pit_rel_lp_loss_fwd_grad_ordered")
        _noise()
        runs.append((norms, loss, dq))
    torch.cuda.synchronize()
    assert not bool(ws.any())
    e_loss = abs(float(runs[0][1]) - float(ref.detach())) / abs(float(ref.detach()))
    e_dq = _err(runs[0][2], q64.grad)
    print("ordered loss", (b, npts, nch, p), e_loss, e_dq)
    assert e_loss <= 1e-6 and e_dq <= TOL
    for other in runs[1:]:
        for a, o in zip(runs[0], other):
            assert torch.equal(a, o)


# --------------------------------------------------------------------------- 4. models
def _darcy_like(seed=5):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    model = tasks.pit_darcy(2, 1, 1, 32, 2, 2, tasks.grid_mesh_2d(8, True, "cuda"), 0.05, 0.05).cuda()
    g = torch.Generator().manual_seed(seed)
    mesh = (tasks.grid_mesh_2d(16, True) + 0.01 * torch.rand(16, 16, 2, generator=g)).cuda()
    f, tgt = torch.randn(3, 16, 16, 1, generator=g).cuda(), torch.randn(3, 16, 16, 1, generator=g).cuda()
    return model, (mesh, f, mesh), tgt, (1, 2)


def _burgers_like(seed=6):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    model = tasks.pit_burgers(1, 1, 1, 32, 2, 2, tasks.line_mesh_1d(32, device="cuda"), 0.1, 0.1).cuda()
    g = torch.Generator().manual_seed(seed)
    mesh = tasks.line_mesh_1d(128).cuda()
    return model, (mesh, torch.randn(3, 128, 1, generator=g).cuda(), mesh), torch.randn(3, 128, 1, generator=g).cuda(), (1, 1)


def _elasticity_like(seed=3):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    model = tasks.pit_elasticity(2, 5, 1, 64, 2, 2, None, 0.05, 0.05).cuda()
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(3, 150, 2, generator=g).cuda()
    return model, (xy, torch.randn(3, 150, 5, generator=g).cuda(), xy), torch.randn(3, 150, 1, generator=g).cuda(), (1, 2)


def _cloud_latent_like(seed=8):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    model = tasks.pit_cloud_latent(2, 5, 1, 32, 2, 2, torch.rand(64, 2, generator=g).cuda(), 0.1, 0.1).cuda()
    xy = torch.rand(3, 150, 2, generator=g).cuda()
    return model, (xy, torch.randn(3, 150, 5, generator=g).cuda(), xy), torch.randn(3, 150, 1, generator=g).cuda(), (1, 2)


MODELS = {"darcy": _darcy_like, "burgers": _burgers_like, "elasticity": _elasticity_like, "cloud_latent": _cloud_latent_like}


def _run_model(model, inputs, tgt, lp):
    from position_induced_transformer_amd import utils
    for q in model.parameters():
        q.grad = None
    mesh_in, f, mesh_out = inputs
    f = f.clone().requires_grad_(True)
    out = model(mesh_in, f, mesh_out)
    loss = utils.RelLpNorm(*lp)(tgt, out)
    loss.backward()
    return [out.detach().clone(), loss.detach().clone(), f.grad.clone()] + [q.grad.clone() for q in model.parameters()]


@pytest.mark.parametrize("name", list(MODELS))
def test_models_repeat_bit_for_bit_and_run_only_ordered_launches(name, monkeypatch):
    from position_induced_transformer_amd import ops, pit as P
    model, inputs, tgt, lp = MODELS[name]()
    log = LaunchLog(monkeypatch)
    with ops.reproducible():
        runs = []
        for _ in range(3):
            runs.append(_run_model(model, inputs, tgt, lp))
            _noise()
    torch.cuda.synchronize()
    names = ["out", "loss", "d_func_in"] + [k for k, _ in model.named_parameters()]
    for other in runs[1:]:
        for k, a, b in zip(names, runs[0], other):
            assert torch.equal(a, b), k
    assert not [c for c in log.calls if c in ("pit_mlp_bwd", "pit_mlp_bwd_params") or c.startswith(FUSED)], log.calls
    n_mlp = sum(1 for m in model.modules() if isinstance(m, P.kaiming_mlp))
    assert log.count("pit_mlp_bwd_params_ordered_mfma") == 3 * n_mlp, log.calls
    assert log.count("pit_rel_lp_loss_fwd_grad_ordered") == 3 and not [c for c in log.calls if c in ("pit_rel_lp_loss_fwd", "pit_rel_lp_loss_fwd_grad")]


def test_darcy_like_model_matches_the_oracle_in_the_mode():
    from position_induced_transformer_amd import ops
    model, inputs, tgt, lp = _darcy_like()
    with ops.reproducible(), ops.head_scale_route("host"):
        got = _run_model(model, inputs, tgt, lp)
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    mi = inputs[0].cpu().double().reshape(-1, 2)
    f = orc.with_coords(mi, inputs[1].cpu().double().reshape(3, -1, 1))
    with fp32_keep_oracle():
        ref = orc.pit_apply(p, "euclid", False, 2, 0.05, 0.05, mi, f, model.mesh_ltt.cpu().double(), mi).reshape(3, 16, 16, 1)
    ref_loss = orc.rel_lp_loss(tgt.cpu().double(), ref, *lp)
    ref_loss.backward()
    e_out = _rel(got[0], ref)
    e_loss = abs(float(got[1]) - float(ref_loss)) / abs(float(ref_loss))
    e_w = max(_rel(q.grad, p[k].grad) for k, q in model.named_parameters() if not k.endswith("lmda"))
    e_l = max(_rel(q.grad, p[k].grad) for k, q in model.named_parameters() if k.endswith("lmda"))
    print("darcy-like, mode on:", e_out, e_loss, e_w, e_l)
    assert e_out <= 1e-5 and e_loss <= 1e-5 and e_w <= 2e-5 and e_l <= 2e-4


def test_elasticity_like_model_matches_the_oracle_in_the_mode():
    from position_induced_transformer_amd import ops
    model, inputs, tgt, lp = _elasticity_like()
    with ops.reproducible(), ops.head_scale_route("host"):
        got = _run_model(model, inputs, tgt, lp)
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    xy = inputs[0].cpu().double()
    with fp32_keep_oracle():
        ref = orc.pit_apply(p, "euclid", True, 2, 0.05, 0.05, xy, inputs[1].cpu().double(), xy, xy)
    ref_loss = orc.rel_lp_loss(tgt.cpu().double(), ref.reshape(tgt.shape), *lp)
    ref_loss.backward()
    e_out = _rel(got[0], ref.reshape(got[0].shape))
    e_loss = abs(float(got[1]) - float(ref_loss)) / abs(float(ref_loss))
    e_w = max(_rel(q.grad, p[k].grad) for k, q in model.named_parameters() if not k.endswith("lmda"))
    e_l = max(_rel(q.grad, p[k].grad) for k, q in model.named_parameters() if k.endswith("lmda"))
    print("elasticity-like, mode on:", e_out, e_loss, e_w, e_l)
    assert e_out <= 1e-5 and e_loss <= 1e-5 and e_w <= 2e-5 and e_l <= 2e-4


def _model_errors(model, got, ref, ref_loss, p):
    e_out = _rel(got[0], ref.reshape(got[0].shape))
    e_loss = abs(float(got[1]) - float(ref_loss)) / abs(float(ref_loss))
    e_w = max(_rel(q.grad, p[k].grad) for k, q in model.named_parameters() if not k.endswith("lmda"))
    e_l = max(_rel(q.grad, p[k].grad) for k, q in model.named_parameters() if k.endswith("lmda"))
    return e_out, e_loss, e_w, e_l


def test_burgers_like_model_matches_the_oracle_in_the_mode():
    """The periodic metric (its forward returns before the mesh-gradient refusals)."""
    from position_induced_transformer_amd import ops
    model, inputs, tgt, lp = _burgers_like()
    with ops.reproducible(), ops.head_scale_route("host"):
        got = _run_model(model, inputs, tgt, lp)
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    mi = inputs[0].cpu().double()
    f = orc.with_coords(mi, inputs[1].cpu().double())
    with fp32_keep_oracle():
        ref = orc.pit_apply(p, "periodic1d", False, 2, 0.1, 0.1, mi, f, model.mesh_ltt.cpu().double(), mi)
    ref_loss = orc.rel_lp_loss(tgt.cpu().double(), ref, *lp)
    ref_loss.backward()
    e_out, e_loss, e_w, e_l = _model_errors(model, got, ref, ref_loss, p)
    print("burgers-like, mode on:", e_out, e_loss, e_w, e_l)
    assert e_out <= 1e-5 and e_loss <= 1e-5 and e_w <= 2e-5 and e_l <= 2e-4


def test_cloud_latent_model_matches_the_oracle_in_the_mode():
    """Per-sample clouds against the latent mesh shared by the batch: the mixed pairs and the batch-free processor."""
    from position_induced_transformer_amd import ops
    model, inputs, tgt, lp = _cloud_latent_like()
    with ops.reproducible(), ops.head_scale_route("host"):
        got = _run_model(model, inputs, tgt, lp)
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    xy = inputs[0].cpu().double()
    with fp32_keep_oracle():
        ref = orc.pit_apply(p, "euclid", True, 2, 0.1, 0.1, xy, inputs[1].cpu().double(), model.mesh_ltt.cpu().double()[None], xy)
    ref_loss = orc.rel_lp_loss(tgt.cpu().double(), ref.reshape(tgt.shape), *lp)
    ref_loss.backward()
    e_out, e_loss, e_w, e_l = _model_errors(model, got, ref, ref_loss, p)
    print("cloud-latent, mode on:", e_out, e_loss, e_w, e_l)
    assert e_out <= 1e-5 and e_loss <= 1e-5 and e_w <= 2e-5 and e_l <= 2e-4


NEW_ENTRIES = ("pit_mlp_bwd_params_ordered_mfma", "pit_lists_sort_ranges", "pit_posatt_overflow_dv_ordered",
               "pit_rel_lp_loss_fwd_grad_ordered")


def test_switch_is_inert_when_off(monkeypatch):
    """Mode off: the fused launches are still taken and none of the new entry points is called.  The Darcy-like model of this
    file (hid 32, 64 latent points, batch 3) is outside the envelope of the fused launches whatever the switch says -
    pit_block_supported wants hid 64 and a multiple of 256 latent points, pit_edge_supported at least 256 rows (3 x 64 = 192 on
    the encoder side), and 64 keys are too few for candidate lists (3 * capacity > 64), which the fused decoder needs - so the
    three launches are looked for on the Darcy configuration itself (43^2 -> 16^2, hid 64) at batch 2; the Darcy-like model
    must call none of the new entries."""
    from position_induced_transformer_amd import ops, tasks
    assert not ops.get_reproducible()
    model, inputs, tgt, lp = _darcy_like()
    full, sample, _ = tasks.make_task("darcy", seed=0)
    mesh_in, func_in, mesh_out, _t = sample(2)
    log = LaunchLog(monkeypatch)
    model(*inputs).sum().backward()
    torch.cuda.synchronize()
    assert log.calls and not [c for c in log.calls if c in NEW_ENTRIES], log.calls
    log.calls.clear()
    full(mesh_in, func_in, mesh_out).sum().backward()
    torch.cuda.synchronize()
    for name in ("pit_encoder_fwd", "pit_block_fwd", "pit_decoder_fwd"):
        assert log.count(name) >= 1, log.calls
    assert not [c for c in log.calls if c in NEW_ENTRIES], log.calls


def test_bf16_mode_is_refused_before_any_launch(monkeypatch):
    from position_induced_transformer_amd import ops
    model, inputs, tgt, lp = _darcy_like()
    log = LaunchLog(monkeypatch)
    with ops.math_mode("bf16"), ops.reproducible():
        with pytest.raises(NotImplementedError, match="reproducible"):
            model(*inputs)
    assert log.calls == []


def test_captured_training_is_the_same_bits_for_two_models_from_one_seed():
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    from position_induced_transformer_amd.engine import TrainStep
    vecs = []
    with ops.reproducible():
        for _ in range(2):
            model, inputs, tgt, lp = _darcy_like(seed=9)
            flat = FlatGradients(model.parameters(), flatten_params=True)
            step = TrainStep(model, (inputs[0], inputs[1], inputs[2], tgt), lp[0], lp[1], optimizer=FlatAdam(flat, lr=1e-3), flat=flat)
            step.capture()
            for _ in range(3):
                step.replay()
                _noise()
            torch.cuda.synchronize()
            vecs.append(torch.cat([q.detach().reshape(-1) for q in model.parameters()]).clone())
    assert torch.isfinite(vecs[0]).all() and torch.equal(vecs[0], vecs[1])

