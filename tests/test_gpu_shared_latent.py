"""GPU: per-sample clouds against ONE mesh shared by the whole batch (a (n, s) mesh paired with a (b, n', s) mesh).

Reference for every comparison: the oracle called ONCE PER SAMPLE on (shared mesh as mesh[None], the cloud truncated to len[s]) as a
batch of one - fp32 for values and kept sets; gradients against the same per-sample oracle evaluated in fp64 with the kept sets of its
fp32 twin (the convention of tests/test_gpu_ragged.py).  Weight and lmda gradients of a batch are compared with the SUM over samples.
Tolerances are the project's: kept sets exact, forward 1e-6 per layer and 1e-5 at model level, d_values / MLP gradients 1e-5 (2e-5 at
model level), d_lmda 1e-4 (2e-4 at model level), all relative to max|ref| per tensor."""
import contextlib

import pytest
import torch

import pit_oracle as orc

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL, LMDA_TOL = 1e-6, 1e-5, 1e-4
M_FWD_TOL, M_GRAD_TOL, M_LMDA_TOL = 1e-5, 2e-5, 2e-4
WIDTH, LENGTHS = 150, [150, 97, 40]


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


def _shared_mesh(n, sd, g):
    """64 points: an 8 x 8 grid plus jitter (2-d only); otherwise n random points."""
    if n == 64 and sd == 2:
        ax = torch.linspace(0, 1, 8)
        grid = torch.stack(torch.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
        return (grid + 0.02 * torch.randn(64, 2, generator=g)).contiguous()
    return torch.rand(n, sd, generator=g)


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


def _oracle_layer(orient, shared, cloud, x, lmda, loc, dy, lens, dtype):
    """Per-sample oracle of a mixed layer: outputs, d_values (per sample), the summed d_lmda and the attention weights."""
    outs, dvs, atts = [], [], []
    dl = torch.zeros_like(lmda, dtype=dtype)
    for s, n in enumerate(lens):
        lm = lmda.detach().to(dtype).requires_grad_(True)
        sh, cl = shared[None].to(dtype), cloud[s:s + 1, :n].to(dtype)
        if orient == "rows":                                   # shared rows, cloud keys
            a, c, xs, g = sh, cl, x[s:s + 1, :n], dy[s:s + 1]
        else:                                                  # cloud rows, shared keys
            a, c, xs, g = cl, sh, x[s:s + 1], dy[s:s + 1, :n]
        xs = xs.to(dtype).requires_grad_(True)
        o = orc.posatt_cross("euclid", True, a, c, xs, lm, loc)
        gv, gl = torch.autograd.grad(o, (xs, lm), g.to(dtype))
        outs.append(o.detach()[0]); dvs.append(gv[0]); dl += gl
        with torch.no_grad():
            atts.append(orc.attention_weights(orc.sqdist("euclid", a, c), orc.head_scale(lm), loc, True)[0])
    return outs, dvs, dl, atts


def _run_layer(mod, orient, shared, cloud, x, dy, lens):
    """The mixed layer on the GPU; ``lens`` None = no lengths.  Returns out, d_values, d_lmda, the plan-free dist2att matrix."""
    sh, cl = shared.cuda(), cloud.cuda()
    x = x.cuda().requires_grad_(True)
    mod.lmda.grad = None
    if orient == "rows":
        mo, mi, kw = sh, cl, ({} if lens is None else {"len_in": lens})
    else:
        mo, mi, kw = cl, sh, ({} if lens is None else {"len_out": lens})
    out = mod(mo, mi, x, **kw)
    out.backward(dy.cuda())
    with torch.no_grad():
        att = mod.dist2att(mo, mi, mod.lmda, mod.locality, **kw)
    return out.detach().cpu(), x.grad.cpu(), mod.lmda.grad.detach().cpu(), att.cpu()


def _check_layer(orient, heads, dim, sd, n_shared, loc, lengths, width, with_lengths, seed):
    from position_induced_transformer_amd import pit
    b = len(lengths)
    g = torch.Generator().manual_seed(seed)
    real = lengths if with_lengths else [width] * b
    shared = _shared_mesh(n_shared, sd, g)
    cloud = _cloud(b, width, sd, g, real)
    n_out, n_in = (n_shared, width) if orient == "rows" else (width, n_shared)
    x = _vals(b, n_in, dim, g, real) if orient == "rows" else torch.randn(b, n_in, dim, generator=g)
    dy = torch.randn(b, n_out, heads * dim, generator=g)
    mod = pit.posatt_cross(heads, dim, loc).cuda()
    out, dv, dl, att = _run_layer(mod, orient, shared, cloud, x, dy, lengths if with_lengths else None)
    lmda = mod.lmda.detach().cpu()
    ref32, _, _, ratt = _oracle_layer(orient, shared, cloud, x, lmda, loc, dy, real, torch.float32)
    with fp32_keep_oracle():
        _, rdv, rdl, _ = _oracle_layer(orient, shared, cloud, x, lmda, loc, dy, real, torch.float64)
    assert out.shape == (b, n_out, heads * dim) and dv.shape == (b, n_in, dim)
    for s, n in enumerate(real):
        lo, li = (n_out, n) if orient == "rows" else (n, n_in)
        e_out, e_dv = _err(out[s, :lo], ref32[s]), _err(dv[s, :li], rdv[s])
        print(f"sample {s} ({n} points): forward {e_out:.2e} d_values {e_dv:.2e}")
        assert torch.equal(att[s, :, :lo, :li] > 0, ratt[s] > 0), f"kept sets of sample {s}"
        assert _err(att[s, :, :lo, :li], ratt[s]) <= FWD_TOL
        assert e_out <= FWD_TOL
        assert e_dv <= GRAD_TOL
        assert torch.all(out[s, lo:] == 0) and torch.all(att[s, :, lo:] == 0)       # padded rows: zero
        assert torch.all(dv[s, li:] == 0) and torch.all(att[s, :, :, li:] == 0)     # padded keys: zero d_values
    e_dl = _err(dl, rdl)
    print(f"d_lmda {e_dl:.2e}")
    assert e_dl <= LMDA_TOL


# (heads, dim, space_dim, shared points): 2 heads with hid 32 and 1 head with hid 3; space_dim 1, 2 and 3; 64 and 100 shared points.
# Shared KEYS at locality 0.05 need 100 points for candidate lists (64 keys: capacity 32 is not a third of the row - dense masked).
SHAPES = {("rows", 0.05): (2, 32, 2, 64), ("rows", 0.3): (1, 3, 1, 100), ("rows", 1.0): (2, 32, 3, 100),
          ("keys", 0.05): (2, 32, 3, 100), ("keys", 0.3): (2, 32, 2, 64), ("keys", 1.0): (1, 3, 1, 64)}


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
@pytest.mark.parametrize("loc", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("orient", ["rows", "keys"])
def test_layer_matrix(orient, loc, with_lengths):
    """{shared rows / cloud keys, cloud rows / shared keys} x {lists, dense masked, dense} x {with lengths, without}: forward,
    d_values, d_lmda and the kept sets through dist2att."""
    from position_induced_transformer_amd import ops
    heads, dim, sd, n_shared = SHAPES[(orient, loc)]
    n_in = WIDTH if orient == "rows" else n_shared
    cap = ops.ragged_list_capacity(ops.quantile_rank(loc, n_in)[0], n_in) if loc < 1.0 else 0
    assert (cap > 0) == (loc == 0.05)                          # 0.05: candidate lists; 0.3: dense masked (cap == 0); 1.0: dense
    _check_layer(orient, heads, dim, sd, n_shared, loc, LENGTHS, WIDTH, with_lengths, 200 + int(loc * 100) + (orient == "keys"))


@pytest.mark.parametrize("orient", ["rows", "keys"])
def test_length_of_one_and_batch_of_one(orient):
    _check_layer(orient, 2, 32, 2, 100, 0.05, [1, 150, 63], WIDTH, True, 301)
    _check_layer(orient, 1, 3, 3, 64, 0.3, [77], WIDTH, True, 302)


@pytest.mark.parametrize("orient", ["rows", "keys"])
def test_overflowed_lists(orient):
    """A shared mesh with 30 coincident points.  As keys their tie shell (30 keys plus the nearer ones) exceeds the capacity of 32;
    as rows the overflow comes from 40 coincident keys of the first cloud.  With lengths; rows that overflow scan all keys."""
    from position_induced_transformer_amd import ops, pit
    g = torch.Generator().manual_seed(77)
    b, dim, loc, heads = 3, 32, 0.05, 2
    shared = torch.rand(100, 2, generator=g)
    shared[50:80] = shared[50]
    cloud = _cloud(b, WIDTH, 2, g, LENGTHS)
    if orient == "rows":
        cloud[0, :40] = cloud[0, 0]
    sh, cl = shared.cuda(), cloud.cuda()
    mo, mi, kw = (sh, cl, {"len_in": LENGTHS}) if orient == "rows" else (cl, sh, {"len_out": LENGTHS})
    plan = ops.MeshPlan("euclid", mo, mi, loc, False, **kw)
    assert plan.nbr_idx is not None and plan.nbr_cap == 32
    over = (plan.nbr_cnt > plan.nbr_cap).cpu()
    assert over.any(), "no row overflowed its list"
    if orient == "keys":
        assert all((plan.nbr_cnt.cpu()[s, n:] == 0).all() for s, n in enumerate(LENGTHS))     # padded rows: empty lists
    n_out, n_in = plan.n_out, plan.n_in
    x = _vals(b, n_in, dim, g, LENGTHS) if orient == "rows" else torch.randn(b, n_in, dim, generator=g)
    dy = torch.randn(b, n_out, heads * dim, generator=g)
    mod = pit.posatt_cross(heads, dim, loc).cuda()
    out, dv, dl, att = _run_layer(mod, orient, shared, cloud, x, dy, LENGTHS)
    lmda = mod.lmda.detach().cpu()
    ref32, _, _, ratt = _oracle_layer(orient, shared, cloud, x, lmda, loc, dy, LENGTHS, torch.float32)
    with fp32_keep_oracle():
        _, rdv, rdl, _ = _oracle_layer(orient, shared, cloud, x, lmda, loc, dy, LENGTHS, torch.float64)
    for s, n in enumerate(LENGTHS):
        lo, li = (n_out, n) if orient == "rows" else (n, n_in)
        assert torch.equal(att[s, :, :lo, :li] > 0, ratt[s] > 0), f"sample {s}"
        assert _err(out[s, :lo], ref32[s]) <= FWD_TOL and _err(dv[s, :li], rdv[s]) <= GRAD_TOL
        assert torch.all(out[s, lo:] == 0) and torch.all(dv[s, li:] == 0)
    assert _err(dl, rdl) <= LMDA_TOL


@pytest.mark.parametrize("loc", [0.05, 1.0])
@pytest.mark.parametrize("orient", ["rows", "keys"])
def test_equivalent_to_expansion(orient, loc):
    """Without lengths: bit-identical to the same module called with shared.expand(b, -1, -1).contiguous().  With lengths:
    bit-identical to the existing ragged call with the expanded mesh and len = [n] * b on the shared side.  Same list capacity."""
    from position_induced_transformer_amd import ops, pit
    g = torch.Generator().manual_seed(55)
    b, dim, heads, n = 3, 32, 2, 100
    shared = torch.rand(n, 2, generator=g).cuda()
    cloud = _cloud(b, WIDTH, 2, g, LENGTHS).cuda()
    expanded = shared.expand(b, -1, -1).contiguous()
    x = (_vals(b, WIDTH, dim, g, LENGTHS) if orient == "rows" else torch.randn(b, n, dim, generator=g)).cuda()
    mod = pit.posatt_cross(heads, dim, loc).cuda()
    full = [n] * b
    with torch.no_grad():
        if orient == "rows":
            plain, plain_x = mod(shared, cloud, x), mod(expanded, cloud, x)
            rag, rag_x = mod(shared, cloud, x, len_in=LENGTHS), mod(expanded, cloud, x, len_out=full, len_in=LENGTHS)
            plans = (ops.MeshPlan("euclid", shared, cloud, loc, False, len_in=LENGTHS),
                     ops.MeshPlan("euclid", expanded, cloud, loc, False, len_out=full, len_in=LENGTHS),
                     ops.MeshPlan("euclid", shared, cloud, loc, False), ops.MeshPlan("euclid", expanded, cloud, loc, False))
        else:
            plain, plain_x = mod(cloud, shared, x), mod(cloud, expanded, x)
            rag, rag_x = mod(cloud, shared, x, len_out=LENGTHS), mod(cloud, expanded, x, len_out=LENGTHS, len_in=full)
            plans = (ops.MeshPlan("euclid", cloud, shared, loc, False, len_out=LENGTHS),
                     ops.MeshPlan("euclid", cloud, expanded, loc, False, len_out=LENGTHS, len_in=full),
                     ops.MeshPlan("euclid", cloud, shared, loc, False), ops.MeshPlan("euclid", cloud, expanded, loc, False))
    assert torch.equal(plain, plain_x)
    assert torch.equal(rag, rag_x)
    assert plans[0].nbr_cap == plans[1].nbr_cap and plans[2].nbr_cap == plans[3].nbr_cap
    assert (plans[0].nbr_cap > 0) == (loc < 1.0)
    # the ragged plan reads the shared mesh in place: no (b, n, s) copy
    assert (plans[0].mesh_out if orient == "rows" else plans[0].mesh_in).data_ptr() == shared.data_ptr()


# ---- model -----------------------------------------------------------------------------------------------------------------
def _latent(n_side_x, n_side_y, g):
    ax, ay = torch.linspace(0, 1, n_side_x), torch.linspace(0, 1, n_side_y)
    grid = torch.stack(torch.meshgrid(ax, ay, indexing="ij"), -1).reshape(-1, 2)
    return (grid + 0.02 * torch.randn(grid.shape, generator=g)).contiguous()


def _model(hid=32, heads=2, blocks=2, seed=3, loc=0.05):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    ltt = _latent(8, 8, torch.Generator().manual_seed(seed)).cuda()
    return tasks.pit_cloud_latent(2, 1, 1, hid, heads, blocks, ltt, loc, loc).cuda()


def _oracle_model(model, mesh, func, target, lengths, dtype, params=None, blocks=2):
    """Per-sample oracle of the model + RelLpNorm(p=2): predictions, summed loss, summed parameter gradients."""
    if params is None:
        params = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in model.state_dict().items()}
    ltt = model.mesh_ltt.detach().cpu().to(dtype)[None]
    preds, loss = [], 0.0
    for s, n in enumerate(lengths):
        m, f, t = mesh[s:s + 1, :n].to(dtype), func[s:s + 1, :n].to(dtype), target[s:s + 1, :n].to(dtype)
        p = orc.pit_apply(params, "euclid", True, blocks, model.en_local, model.de_local, m, f, ltt, m)
        preds.append(p.detach())
        loss = loss + orc.rel_lp_loss(t, p, 1, 2)
    grads = torch.autograd.grad(loss, list(params.values())) if dtype == torch.float64 else None
    return preds, loss.detach(), dict(zip(params.keys(), grads)) if grads is not None else None


def _hip_model_step(model, mesh, func, target, lengths):
    from position_induced_transformer_amd import utils
    for p in model.parameters():
        p.grad = None
    mesh = mesh.cuda()
    if lengths is None:
        pred = model(mesh, func.cuda(), mesh)
        loss = utils.RelLpNorm(1, 2)(target.cuda(), pred)
    else:
        pred = model(mesh, func.cuda(), mesh, len_in=lengths)
        loss = utils.RelLpNorm(1, 2)(target.cuda(), pred, lengths)
    loss.backward()
    return pred.detach().cpu(), loss.detach().cpu(), {k: v.grad.detach().cpu() for k, v in model.named_parameters()}


def _check_against_oracle(model, pred, loss, grads, mesh, func, target, real):
    ref32, _, _ = _oracle_model(model, mesh, func, target, real, torch.float32)
    with fp32_keep_oracle():
        ref64, loss64, rg = _oracle_model(model, mesh, func, target, real, torch.float64)
    for s, n in enumerate(real):
        e64, e32 = _err(pred[s, :n], ref64[s][0]), _err(pred[s, :n], ref32[s][0])
        print(f"sample {s} ({n} points): prediction vs fp64 oracle {e64:.2e}, vs fp32 oracle {e32:.2e}")
        assert e64 <= M_FWD_TOL and e32 <= M_FWD_TOL
    e = abs(float(loss) - float(loss64)) / abs(float(loss64))
    print(f"loss {float(loss):.7f} vs {float(loss64):.7f}: {e:.2e}")
    assert e <= M_FWD_TOL
    for k, gref in rg.items():
        e = _err(grads[k], gref)
        print(f"grad {k}: {e:.2e}")
        assert torch.isfinite(grads[k]).all(), k
        assert e <= (M_LMDA_TOL if k.endswith("lmda") else M_GRAD_TOL), k


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
def test_model_vs_per_sample_oracle(with_lengths):
    from position_induced_transformer_amd import tasks
    model = _model()
    real = LENGTHS if with_lengths else [WIDTH] * 3
    mesh, func, target, _ = tasks.ragged_clouds(real, WIDTH, seed=11)
    pred, loss, grads = _hip_model_step(model, mesh, func, target, real if with_lengths else None)
    _check_against_oracle(model, pred, loss, grads, mesh, func, target, real)


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
def test_three_adam_steps_follow_the_oracle(with_lengths):
    from position_induced_transformer_amd import tasks, utils
    model = _model()
    real = [90, 41, 64] if with_lengths else [90] * 3
    mesh, func, target, _ = tasks.ragged_clouds(real, 90, seed=12)
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    ropt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    ltt = model.mesh_ltt.detach().cpu().double()[None]
    for _ in range(3):
        opt.zero_grad(); ropt.zero_grad()
        if with_lengths:
            pred = model(mesh.cuda(), func.cuda(), mesh.cuda(), len_in=real)
            utils.RelLpNorm(1, 2)(target.cuda(), pred, real).backward()
        else:
            pred = model(mesh.cuda(), func.cuda(), mesh.cuda())
            utils.RelLpNorm(1, 2)(target.cuda(), pred).backward()
        opt.step()
        with fp32_keep_oracle():
            loss = 0.0
            for s, n in enumerate(real):
                m = mesh[s:s + 1, :n].double()
                p = orc.pit_apply(ref, "euclid", True, 2, model.en_local, model.de_local, m, func[s:s + 1, :n].double(), ltt, m)
                loss = loss + orc.rel_lp_loss(target[s:s + 1, :n].double(), p, 1, 2)
            loss.backward()
        ropt.step()
    for k, v in model.state_dict().items():
        e = _err(v, ref[k])
        print(f"{k}: {e:.2e}")
        assert e <= (5e-4 if k.endswith("lmda") else 1e-4), k      # the bounds of tests/test_gpu_ragged.py after Adam steps


def test_padding_is_never_read():
    """NaN in the padded part of the clouds - mesh, input function and target: the prediction on real rows is bit-identical to the
    zero-padded run, every gradient is finite and within the tolerances of the oracle."""
    from position_induced_transformer_amd import tasks
    model = _model()
    runs = []
    for fill in (0.0, float("nan")):
        mesh, func, target, _ = tasks.ragged_clouds(LENGTHS, WIDTH, seed=13, pad_value=fill)
        runs.append(_hip_model_step(model, mesh, func, target, LENGTHS))
    (p0, l0, _), (p1, l1, g1) = runs
    for s, n in enumerate(LENGTHS):
        assert torch.isfinite(p1[s, :n]).all() and torch.equal(p0[s, :n], p1[s, :n]), f"sample {s}"
    assert torch.isfinite(l1) and torch.equal(l0, l1)
    mesh, func, target, _ = tasks.ragged_clouds(LENGTHS, WIDTH, seed=13)
    _check_against_oracle(model, p1, l1, g1, mesh, func, target, LENGTHS)


@pytest.mark.parametrize("nx,ny", [(16, 32), (8, 8)], ids=["512", "64"])
def test_processor_is_the_batch_free_processor(monkeypatch, nx, ny):
    """pit.processor on a 2-d latent mesh: bit for bit pit_fixed.processor, through the same library entry points, none ragged."""
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(9)
    mesh = _latent(nx, ny, g).cuda()
    torch.manual_seed(4)
    a = pit.pit(2, 1, 1, 32, 2, 2, mesh, 0.05, 0.05).cuda()
    b = pit.pit_fixed(2, 1, 1, 32, 2, 2, mesh, 0.05, 0.05).cuda()
    b.load_state_dict(a.state_dict())
    f = torch.randn(3, nx * ny, 32, generator=g).cuda()
    log = LaunchLog(monkeypatch)
    with torch.no_grad():
        got = a.processor(f, mesh)
    calls_a = list(log.calls)
    log.calls.clear()
    with torch.no_grad():
        ref = b.processor(f, mesh)
    calls_b = list(log.calls)
    print(calls_a)
    assert torch.equal(got, ref)
    assert calls_a and calls_a == calls_b
    assert not [c for c in calls_a + calls_b if "ragged" in c]
    # ... and with autograd recording, where the backward's launches are chosen in the forward.  One unrecorded pass of each
    # model first: ops memoises host-side queries of the library per shape for the whole process (pit_mlp_bwd_params_deferrable),
    # so whichever model runs a shape first would log one call more than the other
    for m in (a, b):
        m.processor(f.clone().requires_grad_(True), mesh).sum().backward()
        m.zero_grad(set_to_none=True)
    log.calls.clear()
    fa = f.clone().requires_grad_(True)
    a.processor(fa, mesh).sum().backward()
    calls_a = list(log.calls)
    log.calls.clear()
    fb = f.clone().requires_grad_(True)
    b.processor(fb, mesh).sum().backward()
    calls_b = list(log.calls)
    print(calls_a)
    assert calls_a and calls_a == calls_b, (calls_a, calls_b)
    assert not [c for c in calls_a if "ragged" in c]
    assert _err(fa.grad, fb.grad) <= GRAD_TOL
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        if p.grad is not None or q.grad is not None:
            assert _err(p.grad, q.grad) <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), k


def test_self_attention_on_a_2d_mesh_is_posatt_fixed(monkeypatch):
    """posatt.forward(mesh, inputs) with a 2-d mesh: what posatt_fixed.forward computes, the plan from the module's LRU cache."""
    from position_induced_transformer_amd import pit
    g = torch.Generator().manual_seed(10)
    mesh = _latent(8, 8, g).cuda()
    x = torch.randn(3, 64, 32, generator=g).cuda()
    for loc in (1.0, 0.3):
        a, b = pit.posatt(2, 32, loc).cuda(), pit.posatt_fixed(2, 32, loc).cuda()
        b.load_state_dict(a.state_dict())
        with torch.no_grad():
            assert torch.equal(a(mesh, x), b(mesh, x))
            assert len(a._plans) == 1
            plan = next(iter(a._plans.values()))
            a(mesh, x)
            assert len(a._plans) == 1 and next(iter(a._plans.values())) is plan and plan.mesh_batch == 1


def test_one_capture_serves_changing_sizes():
    """forward + loss + backward of the task model captured once; lengths and data overwritten in place; the replay matches the
    oracle of the new sizes (warm-up and stream discipline of tests/test_gpu_ragged.py)."""
    from position_induced_transformer_amd import tasks, utils
    width = 100
    model = _model()
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
    _check_against_oracle(model, pred.detach().cpu(), loss.detach().cpu(), {k: v.detach().cpu() for k, v in grads.items()},
                          m2.cpu(), f2.cpu(), t2.cpu(), second)
    # ... and an eager run of the new sizes, held to the same bounds
    rp, rl, rg = pred.detach().cpu().clone(), loss.detach().cpu().clone(), {k: v.detach().cpu().clone() for k, v in grads.items()}
    ep, el, eg = _hip_model_step(model, m2.cpu(), f2.cpu(), t2.cpu(), second)
    for s, n in enumerate(second):
        assert _err(rp[s, :n], ep[s, :n]) <= M_FWD_TOL
    assert abs(float(rl) - float(el)) <= M_FWD_TOL * abs(float(el))
    for k in eg:
        assert _err(rg[k], eg[k]) <= (M_LMDA_TOL if k.endswith("lmda") else M_GRAD_TOL), k


def test_refusals(monkeypatch):
    """Each raised before any launch."""
    from position_induced_transformer_amd import ops, pit, tasks
    g = torch.Generator().manual_seed(2)
    shared, cloud = torch.rand(20, 2, generator=g).cuda(), torch.rand(2, 30, 2, generator=g).cuda()
    x = torch.randn(2, 30, 4, generator=g).cuda()
    cross, selfa = pit.posatt_cross(1, 4, 0.5).cuda(), pit.posatt(1, 4, 0.5).cuda()
    model = _model()
    log = LaunchLog(monkeypatch)
    with pytest.raises(ValueError, match="shared"):                    # a length for the shared side
        cross(shared, cloud, x, len_out=[20, 20], len_in=[30, 11])
    with pytest.raises(ValueError, match="shared"):
        cross(cloud, shared, torch.randn(2, 20, 4).cuda(), len_out=[30, 11], len_in=[20, 20])
    with pytest.raises(ValueError, match="shared"):
        cross.dist2att(shared, cloud, cross.lmda, 0.5, len_out=[20, 20], len_in=[30, 11])
    with pytest.raises(ValueError, match="shared"):
        model.encoder(cloud, torch.randn(2, 30, 1).cuda(), model.mesh_ltt, len_in=[30, 11], len_ltt=[64, 64])
    with pytest.raises(ValueError, match="shared"):
        model.decoder(model.mesh_ltt, torch.randn(2, 64, 32).cuda(), cloud, len_ltt=[64, 64], len_out=[30, 11])
    for kw in ({}, {"len_in": [30, 11]}):                              # a mesh that requires grad in a mixed pair
        with pytest.raises(NotImplementedError, match="shared mesh against per-sample clouds"):
            cross(shared.clone().requires_grad_(True), cloud, x, **kw)
        with pytest.raises(NotImplementedError, match="shared mesh against per-sample clouds"):
            cross(shared, cloud.clone().requires_grad_(True), x, **kw)
    with pytest.raises(NotImplementedError, match="shared mesh against per-sample clouds"):
        model(cloud.clone().requires_grad_(True), torch.randn(2, 30, 1).cuda(), cloud)
    with pytest.raises(ValueError, match="per-sample"):                # lengths to posatt.forward with a 2-d mesh
        selfa(shared, torch.randn(2, 20, 4).cuda(), lengths=[20, 10])
    with pytest.raises(NotImplementedError, match="bf16"):             # bf16 mode with lengths on a mixed pair
        with ops.math_mode("bf16"):
            cross(shared, cloud, x, len_in=[30, 11])
    with pytest.raises(NotImplementedError, match="bf16"):
        with ops.math_mode("bf16"):
            model(cloud, torch.randn(2, 30, 1).cuda(), cloud, len_in=[30, 11])
    assert log.calls == []


def test_bf16_mode_without_lengths():
    """bf16 math mode, no lengths: the mixed layers run the default kernels, the processor the batch-free one; against the fp32 run
    at the bf16 mode's forward bound of tests/test_gpu_bf16.py (TOL_OUT = 2e-2, relative L2)."""
    from position_induced_transformer_amd import ops, tasks
    model = _model()
    mesh, func, _, _ = tasks.ragged_clouds([WIDTH] * 3, WIDTH, seed=17, device="cuda")
    with torch.no_grad():
        ref = model(mesh, func, mesh)
        with ops.math_mode("bf16"):
            got = model(mesh, func, mesh)
    assert torch.isfinite(got).all() and float((got - ref).norm() / ref.norm()) <= 2e-2
