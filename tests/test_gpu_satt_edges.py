"""GPU: the dense self-attention of the bf16 mode (csrc/pit_satt.hip) at the launch variants the production shapes never reach - an
odd number of 64-row tiles under 128-row workgroups (RT = 2), the split backward (d(values) alone, d(scale) alone), the L = 64 single
tile - and its hand-offs with the MLP chains either side (csrc/pit_chain.hip: y16 = bf16(y) forward, G16 = bf16(d_x / rowsum)
backward), each against a plain high-precision reference of the same operation; and the Vorticity model in bf16 with every one of
these kernels live."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_io as gio
import pit_oracle as orc

pytestmark = pytest.mark.gpu
CANARY = -8531                      # 0xdead as int16: no weight (0 <= w <= 1) has these bits


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _mesh(metric, batched, L, batch, g):
    if metric == "periodic2d":
        side = int(round(L ** 0.5))
        assert side * side == L
        return orc.grid_mesh_2d(side, False).reshape(-1, 2)
    return torch.rand(batch, L, 2, generator=g) if batched else torch.rand(L, 2, generator=g)


def _rt2(L, heads, dim, batch, metric):
    """launch_satt's choice of 128-row workgroups for the forward and the PRE d(scale) (pit_satt.hip: two heads x hid 256, euclid,
    more 64-row tiles x heads than CUs)."""
    return heads == 2 and dim == 256 and metric == "euclid" and batch * ((L + 63) // 64) * heads > 256


# --------------------------------------------------------------------------- 1. the forward's weight tiles, decoded
def _sqdist64(metric, mesh, period):
    """(mesh_batch, L, L) squared distances in fp64 from the fp32 coordinates the kernel reads."""
    m = mesh.double().reshape(-1, mesh.shape[-2], mesh.shape[-1])
    d = (m.unsqueeze(-2) - m.unsqueeze(-3)).abs()
    if metric != "euclid":
        d = torch.minimum(d, float(period) - d)
    return (d ** 2).sum(-1)


def _tile_index(tiles):
    """row and key of every element of ONE (mesh sample, head) tile region [16-row tile T][32-key step s][lane][8]:
    row = 16 T + (lane & 15), key = 32 s + 16 (e >> 2) + 4 (lane >> 4) + (e & 3)."""
    T = np.arange(tiles * 4)[:, None, None, None]
    s = np.arange(tiles * 2)[None, :, None, None]
    lane = np.arange(64)[None, None, :, None]
    e = np.arange(8)[None, None, None, :]
    return np.broadcast_arrays(16 * T + (lane & 15), 32 * s + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3))


TILE_CASES = [   # heads, hid, points, metric, per-sample meshes, batch
    (2, 256, 64, "euclid", True, 128),       # one tile: 256 workgroups of 64 rows
    (2, 256, 64, "euclid", True, 130),       # ... 130 x 1 x 2 > 256: 128-row workgroups, the single tile is odd
    (2, 256, 64, "euclid", False, 130),
    (2, 256, 400, "euclid", True, 18),       # 7 tiles: 18 x 7 x 2 = 252
    (2, 256, 400, "euclid", True, 19),       # 266 > 256: RT = 2
    (2, 256, 400, "euclid", False, 19),
    (2, 256, 1088, "euclid", True, 7),       # 17 tiles: 238
    (2, 256, 1088, "euclid", True, 8),       # 272: RT = 2
    (2, 256, 1088, "euclid", False, 8),
    (2, 256, 400, "periodic2d", False, 19),  # 20 x 20 periodic: odd tiles, 64-row workgroups
    (1, 256, 400, "euclid", True, 19),
    (2, 128, 400, "euclid", True, 19),
]


@pytest.mark.parametrize("heads,dim,L,metric,batched,batch", TILE_CASES)
def test_forward_weight_tiles_hold_the_rounded_weights_and_stay_in_their_buffer(heads, dim, L, metric, batched, batch):
    """pit_satt_fwd's e_tiles through the raw ABI: every (row < L, key < L) weight is bf16(exp(-c m)) of the fp64 formula within one
    bf16 ulp, keys [L, 64 tiles) are exact zeros, and nothing is written past (mesh_batch, heads, pit_satt_tiles_elems(L)) - a guard
    of one more sample's region (at least the 4 x nsteps KB a workgroup's upper waves could spill) keeps its canary."""
    from position_induced_transformer_amd import _lib, ops
    g = torch.Generator().manual_seed(1000 * heads + L + batch)
    mesh = _mesh(metric, batched, L, batch, g)
    plan = ops.MeshPlan(metric, mesh.cuda(), mesh.cuda(), 1.0, True)
    mb, tiles = plan.mesh_batch, (L + 63) // 64
    nsteps = tiles * 2
    lib = _lib.lib()
    assert lib.pit_satt_supported(L, heads, dim, batch, mb)
    elems = int(lib.pit_satt_tiles_elems(L))
    assert elems == tiles * 4 * nsteps * 512
    guard = max(4 * nsteps * 512, heads * elems)
    et = torch.full((mb * heads * elems + guard,), CANARY, dtype=torch.int16, device="cuda")
    c = torch.tensor([1.3, 5.7][:heads], dtype=torch.float32)
    values = torch.randn(batch, L, dim, generator=g).cuda()
    x16 = torch.empty((batch, L, dim), dtype=torch.bfloat16, device="cuda")
    out = torch.empty((batch, L, (1 + heads) * dim), device="cuda")
    rowstat = torch.empty((mb, heads, L, 4), device="cuda")
    scale = torch.empty((heads,), device="cuda")
    cd = c.cuda()
    rc = lib.pit_satt_fwd(plan.mesh_in.data_ptr(), mb, L, plan.sdim, plan.metric_id, plan.period, values.data_ptr(), values.stride(1),
                          values.stride(0), batch, dim, cd.data_ptr(), heads, 1, x16.data_ptr(), out.data_ptr(), out.stride(1),
                          out.stride(0), dim, 1, rowstat.data_ptr(), scale.data_ptr(), et.data_ptr(), 0, _lib.stream_ptr())
    _lib.check(rc, "pit_satt_fwd")
    torch.cuda.synchronize()
    buf = et.cpu().numpy()
    spill = np.flatnonzero(buf[mb * heads * elems:] != CANARY)
    assert spill.size == 0, f"{spill.size} elements written past the tile buffer (first at +{spill[0]}; RT=2: {_rt2(L, heads, dim, batch, metric)})"
    rows, keys = _tile_index(tiles)
    m64 = _sqdist64(metric, plan.mesh_in.cpu(), plan.period)
    regions = buf[:mb * heads * elems].reshape(mb, heads, tiles * 4, nsteps, 64, 8)
    for s in range(mb):
        for h in range(heads):
            dense = np.empty((tiles * 64, tiles * 64), np.int16)
            dense[rows, keys] = regions[s, h]
            ref = torch.exp(-float(c[h]) * m64[s]).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int32)
            got = dense[:L, :L].astype(np.int32)
            ulps = np.abs(got - ref)
            assert ulps.max() <= 1, (s, h, int(ulps.max()), np.argwhere(ulps > 1)[:4].tolist())
            assert (dense[:L, L:] == 0).all(), (s, h, "padding keys not zero")
    # (and the forward these tiles came from: the concat's input columns are exact)
    assert torch.equal(out[..., :dim].cpu(), values.cpu())


# --------------------------------------------------------------------------- 3. the launch variants through posatt_apply
MATRIX = [   # metric, per-sample meshes, points, hid, heads, batch
    ("euclid", True, 400, 256, 2, 19),       # odd tiles under RT = 2: forward, PRE d(values), PRE2 d(scale)
    ("euclid", False, 400, 256, 2, 19),
    ("euclid", True, 1088, 256, 2, 8),
    ("periodic2d", False, 400, 256, 2, 19),  # periodic: 64-row forward / d(scale), the PRE d(values) at RT = 2 on odd tiles
    ("euclid", True, 64, 256, 2, 130),       # the single tile at RT = 2
]
GRADS = {"both": (True, True), "lmda_frozen": (True, False), "values_no_grad": (False, True)}


@pytest.mark.parametrize("metric,batched,L,dim,heads,batch", MATRIX)
def test_dense_self_attention_launch_variants_against_the_oracle(metric, batched, L, dim, heads, batch):
    """posatt_apply (ops.SATT = "1", bf16 mode) against the oracle's posatt_self with both gradients (the merged backward), with lmda
    frozen (d(values) alone: satt_kernel<..., 1, ..., PRE, RT>) and with values that need no gradient (d(scale) alone, PRE2): output and
    d(values) within 2e-2, d(lmda) within 5e-2; weight tiles on and off give the same output and d(values).  The library entry points
    are counted to show which backward ran."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(7 * L + batch)
    mesh = _mesh(metric, batched, L, batch, g)
    values = torch.randn(batch, L, dim, generator=g)
    lmda = torch.rand(heads, 1, 1, generator=g)
    d_out = torch.randn(batch, L, (1 + heads) * dim, generator=g)
    v0, l0 = values.clone().requires_grad_(True), lmda.clone().requires_grad_(True)
    ref = orc.posatt_self(metric, batched, mesh, v0, l0, 1.0)
    ref.backward(d_out)
    plan = ops.MeshPlan(metric, mesh.cuda(), mesh.cuda(), 1.0, True)
    L_ = ops._lib.lib()
    real_f, real_b = L_.pit_satt_fwd, L_.pit_satt_bwd
    calls = {"fwd": 0, "bwd": []}

    def fwd(*a):
        calls["fwd"] += 1
        return real_f(*a)

    def bwd(*a):                                  # (d_values, dscale, e_tiles) present
        calls["bwd"].append((bool(a[17]), bool(a[21]), bool(a[22])))
        return real_b(*a)

    def run(need_v, need_h, tiles):
        v, lm = values.cuda().requires_grad_(need_v), lmda.cuda().requires_grad_(need_h)
        saved = ops.SATT_TILES
        ops.SATT_TILES = tiles
        try:
            out = ops.posatt_apply(v, lm, plan, heads, concat=True)
            out.backward(d_out.cuda())
        finally:
            ops.SATT_TILES = saved
        torch.cuda.synchronize()
        return out.detach(), v.grad, lm.grad

    saved = ops.SATT
    L_.pit_satt_fwd, L_.pit_satt_bwd = fwd, bwd
    try:
        with ops.math_mode("bf16"), ops.head_scale_route("host"):
            ops.SATT = "1"
            assert L_.pit_satt_supported(L, heads, dim, batch, plan.mesh_batch)
            res = {}
            for name, (need_v, need_h) in GRADS.items():
                for tiles in (True, False):
                    calls["bwd"].clear()
                    res[name, tiles] = run(need_v, need_h, tiles)
                    assert calls["bwd"] == [(need_v, need_h, tiles)], (name, tiles, calls["bwd"])
            assert calls["fwd"] == 2 * len(GRADS)
    finally:
        ops.SATT = saved
        L_.pit_satt_fwd, L_.pit_satt_bwd = real_f, real_b
    for name, (need_v, need_h) in GRADS.items():
        out, dv, dl = res[name, True]
        out_off, dv_off, dl_off = res[name, False]
        assert torch.equal(out[..., :dim].cpu(), values), name
        assert _rel(out[..., dim:], ref[..., dim:]) <= 2e-2, (name, _rel(out[..., dim:], ref[..., dim:]))
        assert _rel(out_off, out) <= 1e-6, name
        if need_v:
            assert _rel(dv, v0.grad) <= 2e-2, (name, _rel(dv, v0.grad))
            assert _rel(dv_off, dv) <= 1e-6, (name, _rel(dv_off, dv))
        else:
            assert dv is None and dv_off is None
        if need_h:
            for got in (dl, dl_off):
                err = float((got.cpu().reshape(-1) - l0.grad.reshape(-1)).norm())
                assert err <= 5e-2 * float(l0.grad.norm()), (name, err / float(l0.grad.norm()))
        else:
            assert dl is None and dl_off is None


# --------------------------------------------------------------------------- 4. the hand-offs: mlp_apply -> posatt_apply -> mlp_apply
HANDOFF = {   # metric, mesh, heads, hid, batch (rows = batch x points >= 1024: the chains' minimum)
    "vorticity": ("periodic2d", 256, 2, 256, 4),      # one 16 x 16 periodic mesh
    "cloud": ("euclid", 400, 1, 256, 3),              # a batch-free cloud, one head
}


def _handoff_case(kind):
    metric, L, H, d, b = HANDOFF[kind]
    g = torch.Generator().manual_seed(len(kind) + L)
    mesh = _mesh(metric, False, L, b, g)
    n0 = (1 + H) * d
    t = dict(x=torch.randn(b, L, n0, generator=g), lmda=torch.rand(H, 1, 1, generator=g), d_z=torch.randn(b, L, d, generator=g))
    for i in range(2):
        t[f"w1_{i}"] = torch.randn(d, n0, generator=g) * (2.0 / n0) ** 0.5
        t[f"b1_{i}"] = 0.1 * torch.randn(d, generator=g)
        t[f"w2_{i}"] = torch.randn(d, d, generator=g) * (2.0 / d) ** 0.5
        t[f"b2_{i}"] = 0.1 * torch.randn(d, generator=g)
    return metric, mesh, H, d, t


def _oracle_block(metric, mesh, H, d, t, edit=None, aux=False, hook=None):
    """fp64: gelu(mlp(x)) -> posatt_self -> gelu(mlp(.)); loss sum(z * d_z) (+ aux = |a[..., d:]|^2); gradients of the leaves and of y."""
    p = {k: v.double().requires_grad_(k not in ("d_z",)) for k, v in t.items()}
    y = F.gelu(orc.mlp(p["x"], p["w1_0"], p["b1_0"], p["w2_0"], p["b2_0"]))
    if edit is not None:
        y = edit(y)
    y.retain_grad()
    a = orc.posatt_self(metric, False, mesh.double(), y, p["lmda"], 1.0)
    if hook is not None:
        a.register_hook(hook)
    extra = (a[..., d:] ** 2).sum() if aux else 0.0
    z = F.gelu(orc.mlp(a, p["w1_1"], p["b1_1"], p["w2_1"], p["b2_1"]))
    ((z * p["d_z"]).sum() + extra).backward()
    return y, a, z, p


def _gpu_block(metric, mesh, H, d, t, fuse=True, rider=True, aux=False, hook=None, snap=None):
    """The same on the HIP path (bf16 mode, SATT = "1"), every parameter opted in to in-place gradient accumulation (the rider needs
    it).  Returns y, a, z, d(y), the parameters; `snap` receives the link's operands at the attention's backward."""
    from position_induced_transformer_amd import ops
    plan = ops.MeshPlan(metric, mesh.cuda(), mesh.cuda(), 1.0, True)
    saved = ops.SATT, ops.SATT_FUSE_PREP, ops.SATT_DW_RIDER
    orig_bwd = ops._PosAtt.backward

    def spy_bwd(ctx, d_out):
        lk = ctx.satt_link
        if snap is not None and lk is not None:
            snap.update(g16=None if lk.get("g16") is None else lk["g16"].clone(), d_out=d_out.detach().clone(),
                        rowstat=lk["rowstat"].clone())
        return orig_bwd(ctx, d_out)

    ops.SATT, ops.SATT_FUSE_PREP, ops.SATT_DW_RIDER = "1", fuse, rider
    ops._PosAtt.backward = staticmethod(spy_bwd)
    try:
        with ops.math_mode("bf16"), ops.head_scale_route("host"):
            x = t["x"].cuda().requires_grad_(True)
            p = {k: torch.nn.Parameter(v.cuda()) for k, v in t.items() if k not in ("x", "d_z")}
            for q in p.values():
                q.grad = torch.zeros_like(q)
                ops.mark_inplace_grad(q, q.grad)
            y = ops.mlp_apply(x, p["w1_0"], p["b1_0"], p["w2_0"], p["b2_0"], out_gelu=True, concat_heads=H)
            dy = {}
            y.register_hook(lambda gr: dy.__setitem__("y", gr.detach().clone()))
            y16 = getattr(y, "_pit_x16", None)
            if snap is not None:
                snap.update(y16=None if y16 is None else y16.clone(), y=y.detach().clone())
            a = ops.posatt_apply(y, p["lmda"], plan, H, concat=True)
            if hook is not None:
                a.register_hook(hook)
            extra = (a[..., d:] ** 2).sum() if aux else 0.0
            z = ops.mlp_apply(a, p["w1_1"], p["b1_1"], p["w2_1"], p["b2_1"], out_gelu=True)
            ((z * t["d_z"].cuda()).sum() + extra).backward()
            torch.cuda.synchronize()
            return y.detach(), a.detach(), z.detach(), dy.get("y"), x.grad, p
    finally:
        ops.SATT, ops.SATT_FUSE_PREP, ops.SATT_DW_RIDER = saved
        ops._PosAtt.backward = orig_bwd


class _Flags:
    """Counts the chain launches and records the hand-off flags on the library entry points."""

    def __init__(self):
        from position_induced_transformer_amd import ops
        self.L = ops._lib.lib()
        self.names = ("pit_satt_fwd", "pit_satt_bwd", "pit_mlp_chain_fwd", "pit_mlp_chain_bwd", "pit_fold_att_fwd", "pit_fold_att_bwd",
                      "pit_fold_weights")
        self.seen = {n: [] for n in self.names}

    def __enter__(self):
        self.real = {n: getattr(self.L, n) for n in self.names}
        for n in self.names:
            def spy(*a, _n=n):
                if _n == "pit_satt_fwd":
                    self.seen[_n].append(int(a[-2]))          # x16_ready
                elif _n == "pit_satt_bwd":
                    self.seen[_n].append(int(a[-3]))          # g16_ready
                else:
                    self.seen[_n].append(1)
                return self.real[_n](*a)
            setattr(self.L, n, spy)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.L, n, self.real[n])


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("kind", list(HANDOFF))
def test_chain_handoff_operands_are_exact(kind):
    """(a) The chain in front writes y16 = bf16(y) bit for bit; the chain behind writes G16 = bf16(d_x_h * rowstat[..., 2]) bit for bit
    (rowstat[..., 2] = 1 / rowsum), and pit_satt_fwd / _bwd take them (x16_ready = g16_ready = 1)."""
    metric, mesh, H, d, t = _handoff_case(kind)
    snap = {}
    with _Flags() as fl:
        _gpu_block(metric, mesh, H, d, t, snap=snap)
    assert fl.seen["pit_satt_fwd"] == [1] and fl.seen["pit_satt_bwd"] == [1], fl.seen
    assert len(fl.seen["pit_mlp_chain_fwd"]) == 2 and len(fl.seen["pit_mlp_chain_bwd"]) == 2
    assert snap["y16"] is not None and torch.equal(_bits(snap["y16"]).reshape(-1), _bits(snap["y"].to(torch.bfloat16)).reshape(-1))
    g16, d_out, rowstat = snap["g16"], snap["d_out"], snap["rowstat"]
    b, L = d_out.shape[:2]
    assert g16 is not None and tuple(g16.shape) == (b, H, L, d)
    inv = rowstat[..., 2]                                                  # (mesh_batch = 1, H, L)
    want = torch.stack([d_out[..., (1 + h) * d:(2 + h) * d] * inv[0, h].unsqueeze(-1) for h in range(H)], dim=1).to(torch.bfloat16)
    assert torch.equal(_bits(g16), _bits(want))


@pytest.mark.parametrize("rider", [True, False])
@pytest.mark.parametrize("kind", list(HANDOFF))
def test_chain_attention_chain_against_fp64(kind, rider):
    """(b) prediction, d(input), d(lmda) and all four weight gradients of both MLPs against the fp64 formula at the bf16 mode's
    tolerances (2e-2 prediction, 5e-2 gradients), with the consuming MLP's weight-gradient reductions riding in the attention's
    backward launch and as a launch of their own."""
    metric, mesh, H, d, t = _handoff_case(kind)
    _y0, _a0, z0, p0 = _oracle_block(metric, mesh, H, d, t)
    _y, _a, z, _dy, dx, p = _gpu_block(metric, mesh, H, d, t, rider=rider)
    assert _rel(z, z0) <= 2e-2
    assert _rel(dx, p0["x"].grad) <= 5e-2
    for k, q in p.items():
        assert _rel(q.grad, p0[k].grad) <= 5e-2, (k, _rel(q.grad, p0[k].grad))


def _halve(g):
    g.mul_(0.5)


@pytest.mark.parametrize("how", ["aux_loss", "inplace_hook"])
@pytest.mark.parametrize("kind", list(HANDOFF))
def test_gradient_accumulated_into_the_chains_d_x_reaches_the_attention(kind, how):
    """(c) The attention output has a second consumer created before the consuming MLP (an auxiliary loss on its head columns: its
    gradient is added to the chain's d_x), or a hook that scales its gradient in place (the attention receives the chain's d_x
    buffer - same address - changed in place).  d(values) must be the SATT_FUSE_PREP = False run's bit for bit (G16 formed from the
    final d_out), d(lmda) the same up to the order of its fp64 atomic sums, and both match the fp64 oracle."""
    metric, mesh, H, d, t = _handoff_case(kind)
    aux, hook = how == "aux_loss", (_halve if how == "inplace_hook" else None)
    y0, _a0, _z0, p0 = _oracle_block(metric, mesh, H, d, t, aux=aux, hook=hook)
    on = _gpu_block(metric, mesh, H, d, t, fuse=True, aux=aux, hook=hook)
    off = _gpu_block(metric, mesh, H, d, t, fuse=False, aux=aux, hook=hook)
    assert torch.equal(on[3], off[3]), f"d(values) differs from the prep-launch run: rel {_rel(on[3], off[3]):.3e}"
    assert _rel(on[5]["lmda"].grad, off[5]["lmda"].grad) <= 1e-6
    assert _rel(on[3], y0.grad) <= 5e-2, _rel(on[3], y0.grad)
    # (ONE layer's d(lmda), with the auxiliary term's 2a in its d_out: sums over (m - mbar)-weighted terms that cancel to a few
    # percent of their size, from bf16 weights and values - 8.7e-2 on Vorticity's layer with the prep launch and the hand-off alike;
    # the single-layer bound of test_folded_decoder_on_per_sample_meshes_one_head is 2e-1)
    assert _rel(on[5]["lmda"].grad, p0["lmda"].grad) <= 1e-1, _rel(on[5]["lmda"].grad, p0["lmda"].grad)


@pytest.mark.parametrize("kind", list(HANDOFF))
def test_values_edited_in_place_before_the_attention_are_what_it_reads(kind):
    """(d) y edited in place (no_grad) between the chain that wrote y16 and the attention: the attention must read the edited values
    (forward only - the chain may have saved y for its backward)."""
    from position_induced_transformer_amd import ops
    metric, mesh, H, d, t = _handoff_case(kind)
    plan = ops.MeshPlan(metric, mesh.cuda(), mesh.cuda(), 1.0, True)
    saved = ops.SATT
    ops.SATT = "1"
    try:
        with _Flags() as fl, torch.no_grad(), ops.math_mode("bf16"), ops.head_scale_route("host"):
            w = [t[k].cuda() for k in ("w1_0", "b1_0", "w2_0", "b2_0")]
            y = ops.mlp_apply(t["x"].cuda(), *w, out_gelu=True, concat_heads=H)
            assert getattr(y, "_pit_x16", None) is not None
            y.mul_(-1.5).add_(0.25)
            a = ops.posatt_apply(y, t["lmda"].cuda(), plan, H, concat=True)
            torch.cuda.synchronize()
    finally:
        ops.SATT = saved
    assert fl.seen["pit_satt_fwd"] == [0], fl.seen         # the chain's y16 is stale: the prep launch rounds the edited values
    ref = orc.posatt_self(metric, False, mesh.double(), y.double().cpu(), t["lmda"].double(), 1.0)
    assert torch.equal(a[..., :d].cpu(), y.cpu())
    assert _rel(a[..., d:], ref[..., d:]) <= 2e-2, _rel(a[..., d:], ref[..., d:])


# --------------------------------------------------------------------------- 5. Vorticity in bf16 with every round-6 kernel live
def test_vorticity_bf16_with_chains_handoffs_and_fold_against_the_oracle():
    """BASELINE config 3 at batch 4 - the smallest batch whose processor rows (4 x 256) the MLP chains take - in the bf16 mode against
    the fp32 oracle at test_bf16_mode_full_size_vs_oracle's tolerances; the spies show the chains, both hand-offs and the fold
    launches ran."""
    from position_induced_transformer_amd import ops, tasks, utils
    TOL_OUT, TOL_GRAD, TOL_HEAD = 2e-2, 5e-2, 5e-2
    batch = 4
    model, sample, meta = tasks.make_task("vorticity", seed=71)
    mesh_in, func_in, mesh_out, target = sample(batch)
    with _Flags() as fl, ops.math_mode("bf16"), ops.head_scale_route("host"):
        out = model(mesh_in, func_in, mesh_out)
        loss = utils.RelLpNorm(meta["out_dim"], meta["p"])(target, out)
        loss.backward()
    torch.cuda.synchronize()
    s = fl.seen
    assert s["pit_mlp_chain_fwd"] and s["pit_mlp_chain_bwd"], s
    assert 1 in s["pit_satt_fwd"] and 1 in s["pit_satt_bwd"], s
    assert s["pit_fold_att_fwd"] and s["pit_fold_att_bwd"] and s["pit_fold_weights"], s
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    mi = mesh_in.cpu().reshape(-1, 2)
    ref = orc.pit_apply(p, "periodic2d", False, 4, 0.02, 0.02, mi, orc.with_coords(mi, func_in.cpu().reshape(batch, -1, 10)),
                        model.mesh_ltt.cpu(), mi, norm_after_enc_proc=True).reshape(out.shape)
    ref_loss = orc.rel_lp_loss(target.cpu(), ref, meta["out_dim"], meta["p"])
    ref_loss.backward()
    assert gio.rel_l2(ref.detach().numpy().reshape(-1), out.detach().cpu().numpy().reshape(-1)) <= TOL_OUT
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= TOL_OUT * abs(float(ref_loss.detach()))
    he, hg, be, bg = [], [], [], []
    for k, q in model.named_parameters():
        e, g = p[k].grad.numpy().reshape(-1), q.grad.cpu().numpy().reshape(-1)
        if k.endswith("lmda"):
            he.append(e); hg.append(g)
        elif k.endswith("bias"):               # (biases in front of an InstanceNorm: judged jointly, singly at 3x - as the model test)
            be.append(e); bg.append(g)
            assert gio.rel_l2(e, g) <= 3 * TOL_GRAD, k
        else:
            assert gio.rel_l2(e, g) <= TOL_GRAD, k
    assert gio.rel_l2(np.concatenate(be), np.concatenate(bg)) <= TOL_GRAD
    assert gio.rel_l2(np.concatenate(he), np.concatenate(hg)) <= TOL_HEAD
