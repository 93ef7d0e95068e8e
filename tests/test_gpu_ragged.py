"""GPU: ragged batches of per-sample clouds (padded tensors + per-sample lengths on the device).

Reference for every comparison: the oracle called ONCE PER SAMPLE on that sample's first n_s points as a batch of one - fp32 for
values and kept sets; gradients against the same per-sample oracle evaluated in fp64 through plain autograd with the kept sets of
its fp32 twin (the convention of tests/test_gpu_mesh_grad.py: a near-tie at the threshold cannot flip a mask between
precisions).  Weight and lmda gradients of a batch are compared with the SUM over samples of the per-sample gradients.
Tolerances are the project's: kept sets bit-exact, forward 1e-6, gradients 1e-5 of max|ref| per tensor, lmda gradients 1e-4."""
import contextlib

import pytest
import torch

import pit_oracle as orc

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL, LMDA_TOL = 1e-6, 1e-5, 1e-4


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@contextlib.contextmanager
def fp32_keep_oracle():
    """orc.sqdist / orc.attention_weights with the keep set decided in fp32 from the fp32 inputs, the weights in the input dtype."""
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


def _lengths(kind, n, b):
    """Mixes of lengths for a padded width n: full width, about half, not multiples of 16 / 64, one very short cloud."""
    base = {"mix": [n, max(1, n // 2 + 1), 3, max(1, n - 7), 2], "one": [1, n, max(1, n // 3)], "full": [n] * b}[kind]
    return [min(n, v) for v in (base * b)[:b]]


def _cloud(b, n, sd, g, lengths, fill=0.0):
    m = torch.full((b, n, sd), fill)
    for s, ns in enumerate(lengths):
        m[s, :ns] = torch.rand(ns, sd, generator=g)
    return m


def _vals(b, n, d, g, lengths, fill=0.0):
    v = torch.full((b, n, d), fill)
    for s, ns in enumerate(lengths):
        v[s, :ns] = torch.randn(ns, d, generator=g)
    return v


def _oracle_layer(self_attn, mo, mi, x, lmda, loc, dy, lo, li, dtype):
    """Per-sample oracle: outputs, d_values (per sample) and the summed d_lmda."""
    outs, dvs = [], []
    dl = torch.zeros_like(lmda, dtype=dtype)
    for s in range(x.shape[0]):
        xs = x[s:s + 1, :li[s]].to(dtype).requires_grad_(True)
        lm = lmda.detach().to(dtype).requires_grad_(True)
        a, c = mo[s:s + 1, :lo[s]].to(dtype), mi[s:s + 1, :li[s]].to(dtype)
        o = orc.posatt_self("euclid", True, a, xs, lm, loc) if self_attn else orc.posatt_cross("euclid", True, a, c, xs, lm, loc)
        gv, gl = torch.autograd.grad(o, (xs, lm), dy[s:s + 1, :lo[s]].to(dtype))
        outs.append(o.detach()); dvs.append(gv); dl += gl
    return outs, dvs, dl


# (kind, heads, space_dim, dim, n_out, n_in, batch, locality, lengths)
CASES = [
    ("cross", 1, 2, 44, 100, 150, 3, 1.0, "mix"),
    ("cross", 2, 3, 64, 70, 200, 5, 0.05, "mix"),
    ("cross", 2, 1, 3, 130, 97, 3, 0.02, "mix"),
    ("cross", 1, 2, 256, 50, 77, 4, 0.3, "mix"),
    ("cross", 3, 2, 44, 64, 128, 1, 0.1, "full"),
    ("cross", 2, 2, 64, 90, 33, 3, 0.5, "one"),
    ("self", 2, 2, 64, 150, 150, 3, 1.0, "mix"),
    ("self", 1, 3, 3, 130, 130, 1, 0.05, "mix"),
    ("self", 2, 3, 256, 200, 200, 5, 0.02, "mix"),
    ("self", 3, 1, 44, 97, 97, 3, 0.3, "one"),
    ("self", 1, 2, 256, 64, 64, 4, 1.0, "mix"),
]


def _run_layer(mod, self_attn, mo, mi, x, dy, lo, li):
    x = x.cuda().requires_grad_(True)
    mod.lmda.grad = None
    if self_attn:
        out = mod(mo.cuda(), x, lengths=lo)
    else:
        out = mod(mo.cuda(), mi.cuda(), x, len_out=lo, len_in=li)
    out.backward(dy.cuda())
    return out.detach().cpu(), x.grad.cpu(), mod.lmda.grad.detach().cpu()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_vs_per_sample_oracle(case):
    from position_induced_transformer_amd import pit
    kind, heads, sd, dim, n_out, n_in, b, loc, lk = case
    self_attn = kind == "self"
    g = torch.Generator().manual_seed(100 + CASES.index(case))
    lo = _lengths(lk, n_out, b)
    li = lo if self_attn else _lengths(lk, n_in, b)[::-1]
    mo = _cloud(b, n_out, sd, g, lo)
    mi = mo if self_attn else _cloud(b, n_in, sd, g, li)
    x = _vals(b, n_in, dim, g, li)
    width = (heads + (1 if self_attn else 0)) * dim
    dy = torch.randn(b, n_out, width, generator=g)
    mod = (pit.posatt if self_attn else pit.posatt_cross)(heads, dim, loc).cuda()
    out, dv, dl = _run_layer(mod, self_attn, mo, mi, x, dy, lo, li)
    lmda = mod.lmda.detach().cpu()
    ref32, _, _ = _oracle_layer(self_attn, mo, mi, x, lmda, loc, dy, lo, li, torch.float32)
    with fp32_keep_oracle():
        _, rdv, rdl = _oracle_layer(self_attn, mo, mi, x, lmda, loc, dy, lo, li, torch.float64)
    col0 = dim if self_attn else 0
    for s in range(b):
        e_out, e_dv = _err(out[s, :lo[s]], ref32[s][0]), _err(dv[s, :li[s]], rdv[s][0])
        print(f"sample {s} n_out {lo[s]} n_in {li[s]}: forward {e_out:.2e} d_values {e_dv:.2e}")
        assert e_out <= FWD_TOL
        assert e_dv <= GRAD_TOL
        assert torch.all(out[s, lo[s]:, col0:] == 0)                 # padded rows: zeros in every head column
        assert torch.all(dv[s, li[s]:] == 0)                         # padded keys: zero gradient, residual included
    e_dl = _err(dl, rdl)
    print(f"d_lmda {e_dl:.2e}")
    assert e_dl <= LMDA_TOL


def _lattice(n_side):
    ax = torch.linspace(0, 1, n_side)
    return torch.stack(torch.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)


@pytest.mark.parametrize("loc", [0.05, 0.3, 1.0])
def test_kept_sets_bit_exact(loc):
    """dist2att with lengths: the > 0 pattern equals the per-sample oracle's, on random clouds, a regular lattice (ties at the
    threshold) and duplicated points."""
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(5)
    n, b = 121, 4
    lo, li = [121, 64, 3, 100], [121, 81, 2, 49]
    mo, mi = torch.zeros(b, n, 2), torch.zeros(b, n, 2)
    lat = _lattice(11)
    mo[0], mi[0] = lat, lat                                             # regular lattice: ties at the threshold
    mo[1, :64], mi[1, :81] = _lattice(8), _lattice(9)
    mo[2, :3], mi[2, :2] = torch.rand(3, 2, generator=g), torch.rand(2, 2, generator=g)
    pts = torch.rand(25, 2, generator=g)
    mo[3, :100], mi[3, :49] = pts.repeat(4, 1), torch.cat((pts, pts[:24]))      # duplicate points
    mod = pit.posatt_cross(2, 4, loc).cuda()
    with torch.no_grad():
        att = mod.dist2att(mo.cuda(), mi.cuda(), mod.lmda, loc, len_out=lo, len_in=li).cpu()
    lmda = mod.lmda.detach().cpu()
    for s in range(b):
        ref = orc.attention_weights(orc.sqdist("euclid", mo[s:s + 1, :lo[s]], mi[s:s + 1, :li[s]]), orc.head_scale(lmda), loc, True)[0]
        got = att[s, :, :lo[s], :li[s]]
        assert torch.equal(got > 0, ref > 0), f"sample {s}"
        assert _err(got, ref) <= FWD_TOL
        assert torch.all(att[s, :, lo[s]:] == 0) and torch.all(att[s, :, :, li[s]:] == 0)


@pytest.mark.parametrize("forced_cap", [None, 16])
def test_overflowed_lists(monkeypatch, forced_cap):
    """Rows whose candidate list overflows - 60 coincident keys (ties far beyond the capacity, as tests/test_gpu_ops.py forces
    it), and a forced capacity of 16 that every row of locality 0.1 overflows - scan all keys of their sample: kept sets bit for
    bit, values and gradients against the per-sample oracle."""
    from position_induced_transformer_amd import ops, pit
    if forced_cap is not None:
        monkeypatch.setattr(ops, "RAGGED_LIST_CAP", forced_cap)
    g = torch.Generator().manual_seed(41)
    b, n_out, n_in, dim, loc = 3, 200, 300, 44, 0.1
    lo, li = [200, 93, 150], [300, 131, 2]
    mo, mi = _cloud(b, n_out, 2, g, lo), _cloud(b, n_in, 2, g, li)
    mi[0, 40:100] = mi[0, 40]                                          # 60 coincident keys in sample 0
    plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), loc, False, len_out=lo, len_in=li)
    assert plan.nbr_idx is not None and plan.nbr_cap == (forced_cap or 48)
    over = (plan.nbr_cnt > plan.nbr_cap).cpu()
    assert over[0].any() and (forced_cap is not None or not over[1].any())
    assert (plan.nbr_cnt.cpu()[1, lo[1]:] == 0).all()                  # padded rows: empty lists
    assert (plan.rev_ptr.cpu()[1, li[1]:] == plan.rev_ptr.cpu()[1, li[1]]).all()       # padded keys: empty ranges
    mod = pit.posatt_cross(2, dim, loc).cuda()
    with torch.no_grad():
        att = mod.dist2att(mo.cuda(), mi.cuda(), mod.lmda, loc, len_out=lo, len_in=li).cpu()
    lmda = mod.lmda.detach().cpu()
    for s in range(b):
        ref = orc.attention_weights(orc.sqdist("euclid", mo[s:s + 1, :lo[s]], mi[s:s + 1, :li[s]]), orc.head_scale(lmda), loc, True)[0]
        assert torch.equal(att[s, :, :lo[s], :li[s]] > 0, ref > 0), f"sample {s}"
    x, dy = _vals(b, n_in, dim, g, li), torch.randn(b, n_out, 2 * dim, generator=g)
    out, dv, dl = _run_layer(mod, False, mo, mi, x, dy, lo, li)
    ref32, _, _ = _oracle_layer(False, mo, mi, x, lmda, loc, dy, lo, li, torch.float32)
    with fp32_keep_oracle():
        _, rdv, rdl = _oracle_layer(False, mo, mi, x, lmda, loc, dy, lo, li, torch.float64)
    for s in range(b):
        assert _err(out[s, :lo[s]], ref32[s][0]) <= FWD_TOL and _err(dv[s, :li[s]], rdv[s][0]) <= GRAD_TOL
        assert torch.all(out[s, lo[s]:] == 0) and torch.all(dv[s, li[s]:] == 0)
    assert _err(dl, rdl) <= LMDA_TOL


def _model(hid, heads=2, blocks=2, seed=3, en_loc=0.05, de_loc=0.05):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    return tasks.pit_elasticity(2, 1, 1, hid, heads, blocks, None, en_loc, de_loc).cuda()


def _oracle_model(model, mesh, func, target, lengths, dtype, blocks=2):
    """Per-sample oracle of the model + RelLpNorm(p=2): predictions, summed loss, summed parameter gradients."""
    params = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in model.state_dict().items()}
    preds, loss = [], 0.0
    for s, n in enumerate(lengths):
        m, f, t = mesh[s:s + 1, :n].to(dtype), func[s:s + 1, :n].to(dtype), target[s:s + 1, :n].to(dtype)
        p = orc.pit_apply(params, "euclid", True, blocks, model.en_local, model.de_local, m, f, m, m)
        preds.append(p.detach())
        loss = loss + orc.rel_lp_loss(t, p, 1, 2)
    grads = torch.autograd.grad(loss, list(params.values()))
    return preds, loss.detach(), dict(zip(params.keys(), grads))


def _hip_model_step(model, mesh, func, target, lengths):
    from position_induced_transformer_amd import utils
    for p in model.parameters():
        p.grad = None
    pred = model(mesh.cuda(), func.cuda(), mesh.cuda(), len_in=lengths)
    loss = utils.RelLpNorm(1, 2)(target.cuda(), pred, lengths)
    loss.backward()
    return pred.detach().cpu(), loss.detach().cpu(), {k: v.grad.detach().cpu() for k, v in model.named_parameters()}


def _check_predictions(pred, ref32, ref64, lengths):
    """Forward bound 1e-6 of max|ref| for a whole model (encoder, blocks, decoder: six attention layers and MLPs).  The fp32
    oracle is itself that far from the exact result after six fp32 layers - measured on MI355X / this host's ATen, per sample:
    fp32 oracle vs its fp64 evaluation 1.3e-7 .. 1.2e-6, kernels vs fp32 oracle 2.4e-7 .. 2.0e-6, kernels vs fp64 evaluation
    1.2e-7 .. 7.7e-7 - so the prediction is held to 1e-6 against the oracle's fp64 evaluation with the kept sets of its fp32 twin (the
    reference the gradients and the loss use); the distance to the fp32 oracle is printed, and bounded by the two errors together."""
    for s, n in enumerate(lengths):
        e64, e32 = _err(pred[s, :n], ref64[s][0]), _err(pred[s, :n], ref32[s][0])
        own = _err(ref32[s][0], ref64[s][0])
        print(f"sample {s} ({n} points): prediction vs fp64 oracle {e64:.2e}, vs fp32 oracle {e32:.2e} (fp32 oracle vs fp64 {own:.2e})")
        assert e64 <= FWD_TOL
        assert e32 <= FWD_TOL + own


def _check_model(model, mesh, func, target, lengths):
    pred, loss, grads = _hip_model_step(model, mesh, func, target, lengths)
    ref32, loss32, _ = _oracle_model(model, mesh, func, target, lengths, torch.float32)
    with fp32_keep_oracle():
        ref64, loss64, rg = _oracle_model(model, mesh, func, target, lengths, torch.float64)
    _check_predictions(pred, ref32, ref64, lengths)
    e = abs(float(loss) - float(loss64)) / abs(float(loss64))
    print(f"loss {float(loss):.7f} vs {float(loss64):.7f}: {e:.2e}")
    assert e <= FWD_TOL
    for k, gref in rg.items():
        e = _err(grads[k], gref)
        print(f"grad {k}: {e:.2e}")
        assert e <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), k


@pytest.mark.parametrize("hid,width,lengths", [(32, 150, [150, 77, 3, 101]), (256, 200, [200, 97, 130])])
def test_model_vs_per_sample_oracle(hid, width, lengths):
    from position_induced_transformer_amd import tasks
    model = _model(hid)
    mesh, func, target, _ = tasks.ragged_clouds(lengths, width, seed=11)
    _check_model(model, mesh, func, target, lengths)


def test_three_adam_steps_follow_the_oracle():
    from position_induced_transformer_amd import tasks, utils
    lengths, width = [90, 41, 64], 90
    model = _model(32)
    mesh, func, target, _ = tasks.ragged_clouds(lengths, width, seed=12)
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    ropt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    for _ in range(3):
        opt.zero_grad(); ropt.zero_grad()
        pred = model(mesh.cuda(), func.cuda(), mesh.cuda(), len_in=lengths)
        utils.RelLpNorm(1, 2)(target.cuda(), pred, lengths).backward()
        opt.step()
        with fp32_keep_oracle():
            loss = 0.0
            for s, n in enumerate(lengths):
                m = mesh[s:s + 1, :n].double()
                p = orc.pit_apply(ref, "euclid", True, 2, model.en_local, model.de_local, m, func[s:s + 1, :n].double(), m, m)
                loss = loss + orc.rel_lp_loss(target[s:s + 1, :n].double(), p, 1, 2)
            loss.backward()
        ropt.step()
    for k, v in model.state_dict().items():
        e = _err(v, ref[k])
        print(f"{k}: {e:.2e}")
        assert e <= (5e-4 if k.endswith("lmda") else 1e-4), k      # the bounds of tests/test_gpu_models.py after Adam steps


def _padding_runs():
    from position_induced_transformer_amd import tasks
    lengths, width = [120, 61, 2, 97], 120
    model = _model(32)
    res = []
    for fill in (0.0, float("nan")):
        mesh, func, target, _ = tasks.ragged_clouds(lengths, width, seed=13, pad_value=fill)
        res.append(_hip_model_step(model, mesh, func, target, lengths))
    return res


def test_padding_never_enters_arithmetic():
    """NaN in the padded part of meshes, input function and target: outputs, loss and EVERY gradient finite and bit-identical to
    the run with zero padding.

    The weight gradients of the pointwise MLPs take part: on the ragged path they are summed in a fixed order
    (pit_mlp_bwd_params_ordered).  The atomic reductions of pit_mlp_bwd_params differ in the last bits between two runs on the
    SAME tensors (measured: up to 1.1e-7 of max|g| on 14 of 22 tensors), which would hide what this test is about."""
    (p0, l0, g0), (p1, l1, g1) = _padding_runs()
    assert torch.isfinite(p1).all() and torch.isfinite(l1)
    assert torch.equal(p0, p1) and torch.equal(l0, l1)
    diff = {}
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        if not torch.equal(g0[k], g1[k]):
            diff[k] = float((g0[k] - g1[k]).abs().max() / g0[k].abs().max())
    print("gradients not bit-identical:", diff)
    assert not diff, diff


def test_padding_in_single_layers():
    """One layer of each kind (dense self attention, masked cross attention on lists) with NaN in the padded meshes, values AND
    d_out: out, d_values and d_lmda bit for bit those of zero padding."""
    from position_induced_transformer_amd import pit
    for self_attn, loc in ((True, 1.0), (False, 0.1)):
        g = torch.Generator().manual_seed(31)
        b, n_out, n_in, dim = 4, 100, 100 if self_attn else 77, 44
        lo = [100, 51, 2, 93]
        li = lo if self_attn else [77, 3, 40, 64]
        mod = (pit.posatt if self_attn else pit.posatt_cross)(2, dim, loc).cuda()
        runs = []
        for fill in (0.0, float("nan")):
            g.manual_seed(31)
            mo = _cloud(b, n_out, 2, g, lo, fill)
            mi = mo if self_attn else _cloud(b, n_in, 2, g, li, fill)
            x = _vals(b, n_in, dim, g, li, fill)
            dy = _vals(b, n_out, (2 + self_attn) * dim, g, lo, fill)
            runs.append(_run_layer(mod, self_attn, mo, mi, x, dy, lo, li))
        for got0, got1, name in zip(runs[0], runs[1], ("out", "d_values", "d_lmda")):
            if name == "out" and self_attn:      # the copied columns of padded rows are copied as they are (NaN stays NaN)
                for s in range(b):
                    assert torch.equal(got0[s, :lo[s]], got1[s, :lo[s]]) and torch.equal(got0[s, lo[s]:, dim:], got1[s, lo[s]:, dim:])
                continue
            assert torch.isfinite(got1).all(), name
            assert torch.equal(got0, got1), (self_attn, name)


@pytest.mark.parametrize("self_attn,loc", [(True, 1.0), (True, 0.3), (True, 0.05), (False, 0.05), (False, 0.4)])
def test_full_lengths_agree_with_no_lengths(self_attn, loc):
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(21)
    b, n_out, n_in, dim = 3, 130, 130 if self_attn else 97, 44
    mo = torch.rand(b, n_out, 2, generator=g)
    mi = mo if self_attn else torch.rand(b, n_in, 2, generator=g)
    x = torch.randn(b, n_in, dim, generator=g)
    mod = (pit.posatt if self_attn else pit.posatt_cross)(2, dim, loc).cuda()
    dy = torch.randn(b, n_out, (2 + self_attn) * dim, generator=g)
    got = _run_layer(mod, self_attn, mo, mi, x, dy, [n_out] * b, [n_in] * b)
    xx = x.cuda().requires_grad_(True)
    mod.lmda.grad = None
    out = mod(mo.cuda(), xx) if self_attn else mod(mo.cuda(), mi.cuda(), xx)
    out.backward(dy.cuda())
    with torch.no_grad():
        a0 = mod.dist2att(mo.cuda(), mi.cuda(), mod.lmda, loc)
        a1 = mod.dist2att(mo.cuda(), mi.cuda(), mod.lmda, loc, len_out=[n_out] * b, len_in=[n_in] * b)
    assert torch.equal(a0 > 0, a1 > 0)
    assert _err(got[0], out) <= FWD_TOL
    assert _err(got[1], xx.grad) <= GRAD_TOL
    assert _err(got[2], mod.lmda.grad) <= LMDA_TOL


def test_one_capture_serves_changing_sizes():
    """forward + loss + backward captured once; lengths and data overwritten in place; the replay matches the oracle."""
    from position_induced_transformer_amd import tasks, utils
    width, b = 100, 3
    model = _model(32)
    first, second = [100, 52, 33], [17, 100, 71]
    mesh, func, target, lens = tasks.ragged_clouds(first, width, seed=14, device="cuda")
    loss_fn = utils.RelLpNorm(1, 2)

    def step():
        for p in model.parameters():
            p.grad = None
        pred = model(mesh, func, mesh, len_in=lens)
        loss = loss_fn(target, pred, lens)
        loss.backward()
        return pred, loss
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                   # warm-up outside the capture (workspaces, parameter grads)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pred, loss = step()
    grads = {k: v.grad for k, v in model.named_parameters()}
    m2, f2, t2, l2 = tasks.ragged_clouds(second, width, seed=15, device="cuda")
    mesh.copy_(m2); func.copy_(f2); target.copy_(t2); lens.copy_(l2)
    graph.replay()
    torch.cuda.synchronize()
    ref32, _, _ = _oracle_model(model, m2.cpu(), f2.cpu(), t2.cpu(), second, torch.float32)
    with fp32_keep_oracle():
        ref64, loss64, rg = _oracle_model(model, m2.cpu(), f2.cpu(), t2.cpu(), second, torch.float64)
    _check_predictions(pred.detach().cpu(), ref32, ref64, second)
    assert abs(float(loss.detach()) - float(loss64)) / abs(float(loss64)) <= FWD_TOL
    for k, gref in rg.items():
        assert _err(grads[k], gref) <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), k


def test_masked_loss_vs_truncated_oracle():
    from position_induced_transformer_amd import utils
    g = torch.Generator().manual_seed(8)
    lengths, width = [70, 1, 33, 64], 70
    for p in (1, 2):
        true, pred = torch.randn(4, width, 3, generator=g), torch.randn(4, width, 3, generator=g)
        q = pred.cuda().requires_grad_(True)
        loss = utils.RelLpNorm(3, p)(true.cuda(), q, lengths)
        loss.backward()
        r = pred.double().requires_grad_(True)
        ref = sum(orc.rel_lp_loss(true[s:s + 1, :n].double(), r[s:s + 1, :n], 3, p) for s, n in enumerate(lengths))
        ref.backward()
        assert abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach()) <= 1e-6
        assert _err(q.grad, r.grad) <= GRAD_TOL
        for s, n in enumerate(lengths):
            assert torch.all(q.grad[s, n:] == 0)


def test_refusals():
    from position_induced_transformer_amd import ops, pit
    m3, m2 = torch.rand(2, 20, 2).cuda(), torch.rand(20, 2).cuda()
    x = torch.randn(2, 20, 4).cuda()
    with pytest.raises(ValueError, match="per-sample"):
        pit.posatt_fixed(1, 4, 0.5).cuda()(m2, x, lengths=[20, 10])
    with pytest.raises(ValueError, match="per-sample"):
        pit.posatt_cross_periodic1d(1, 4, 0.5).cuda()._cross(m2, m2, x, len_out=[20, 10], len_in=[20, 10])
    with pytest.raises(ValueError, match="periodic"):
        ops.MeshPlan("periodic1d", m3, m3, 0.5, True, len_out=[20, 10], len_in=[20, 10])
    with pytest.raises(ValueError, match="both"):
        pit.posatt_cross(1, 4, 0.5).cuda()(m3, m3, x, len_out=[20, 10])
    with pytest.raises(NotImplementedError, match="requires grad"):
        pit.posatt(1, 4, 0.5).cuda()(m3.clone().requires_grad_(True), x, lengths=[20, 10])
    with pytest.raises(NotImplementedError, match="bf16"):
        with ops.math_mode("bf16"):
            pit.posatt(1, 4, 0.5).cuda()(m3, x, lengths=[20, 10])
    with pytest.raises(NotImplementedError, match="space_dim > 3"):
        pit.posatt(1, 4, 0.5).cuda()(torch.rand(2, 20, 5).cuda(), x, lengths=[20, 10])


def test_no_lengths_calls_no_ragged_entry(monkeypatch):
    from position_induced_transformer_amd import tasks, utils
    model = _model(32)
    mesh, func, target, _ = tasks.ragged_clouds([60, 60], 60, seed=16, device="cuda")
    log = LaunchLog(monkeypatch)
    pred = model(mesh, func, mesh)
    utils.RelLpNorm(1, 2)(target, pred).backward()
    assert log.calls and not [c for c in log.calls if "ragged" in c or "ordered" in c]
    log.calls.clear()
    pred = model(mesh, func, mesh, len_in=[60, 31])
    utils.RelLpNorm(1, 2)(target, pred, [60, 31]).backward()
    assert {c for c in log.calls if "ragged" in c} == {"pit_plan_ragged_fwd", "pit_posatt_ragged_fwd", "pit_posatt_ragged_bwd",
                                                      "pit_rel_lp_loss_ragged_fwd", "pit_rel_lp_loss_ragged_bwd"}
    assert "pit_mlp_bwd_params_ordered" in log.calls and "pit_mlp_bwd_params" not in log.calls and "pit_mlp_bwd" not in log.calls
    assert not [c for c in log.calls if c in ("pit_posatt_fwd", "pit_posatt_fwd_job", "pit_posatt_bwd", "pit_plan_fwd", "pit_select_fwd")]
