"""GPU: round 6 - the decoder side with de.mlp1 folded into the values (csrc/pit_fold.hip): the bias-free Linear on the latent
points, the fold attention launches on tall slabs (fp32 and bf16 MFMA flavours), the thin tail, each against the oracle
(pit.py:124-127: de(up(values)))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_io as gio
import pit_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# --------------------------------------------------------------------------- the pieces
@pytest.mark.parametrize("rows_b,rows_j,d,heads", [(3, 256, 256, 2), (2, 100, 128, 1), (5, 64, 64, 2)])
def test_linear_on_the_weights_own_memory_equals_the_per_head_products(rows_b, rows_j, d, heads):
    """ops._Linear reads de.mlp1.weight (hid, H*hid) as an (H*hid, hid) matrix: column n*H + h of the result is
    (V W1_h^T)[:, n] (pit.py:126 restricted to head h's columns); d_x and d_w against fp64."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn(rows_b, rows_j, d, generator=g)
    w1 = torch.randn(d, heads * d, generator=g) / d ** 0.5
    dy = torch.randn(rows_b, rows_j, heads * d, generator=g)
    x0, w0 = x.double().requires_grad_(True), w1.double().requires_grad_(True)
    ref = torch.stack([x0 @ w0[:, h * d:(h + 1) * d].T for h in range(heads)], dim=-1).reshape(rows_b, rows_j, d * heads)
    ref.backward(dy.double())
    x1, w_ = x.cuda().requires_grad_(True), w1.cuda().requires_grad_(True)
    y = ops._Linear.apply(x1, w_, None)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert _rel(y, ref) <= 1e-6
    assert _rel(x1.grad, x0.grad) <= 1e-6
    assert _rel(w_.grad, w0.grad) <= 2e-6


@pytest.mark.parametrize("rows,n1,n2,bf16", [(4096, 256, 1, False), (1234, 128, 4, False), (777, 64, 3, False), (4096, 256, 1, True)])
def test_thin_tail_against_torch(rows, n1, n2, bf16):
    """y = gelu(z + b1) W2^T + b2 (pit.py:21-26 after the first Linear) and its backward - dz, d_b1, d_w2, d_b2 - against fp64."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(11)
    z = torch.randn(2, rows // 2, n1, generator=g)
    b1, w2, b2 = torch.randn(n1, generator=g), torch.randn(n2, n1, generator=g) / n1 ** 0.5, torch.randn(n2, generator=g)
    dy = torch.randn(2, rows // 2, n2, generator=g)
    zin = z.to(torch.bfloat16).float() if bf16 else z
    t0 = [t.double().requires_grad_(True) for t in (zin, b1, w2, b2)]
    ref = F.linear(F.gelu(t0[0] + t0[1]), t0[2], t0[3])
    ref.backward(dy.double())
    t1 = [t.cuda().requires_grad_(True) for t in (zin, b1, w2, b2)]
    zz = t1[0].to(torch.bfloat16) if bf16 else t1[0]
    y = ops._ThinTail.apply(zz, t1[1], t1[2], t1[3], (None, None, None))
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert _rel(y, ref) <= 1e-6
    tol = 6e-3 if bf16 else 1e-5                  # (bf16: dz leaves as bf16)
    assert _rel(t1[0].grad, t0[0].grad) <= tol
    for got, want in zip(t1[1:], t0[1:]):
        assert _rel(got.grad, want.grad) <= 1e-5, (got.shape, _rel(got.grad, want.grad))


# --------------------------------------------------------------------------- the folded decoder against the oracle
CASES = [
    ("periodic2d", 64, 16, 256, 2, 2, 0.02, 1),          # Vorticity's decoder (train_vorticity.py:98-106): 256-row slabs, unions of 64
    ("euclid", 43, 16, 128, 1, 3, 0.02, 3),              # 1849 rows: the mesh ends inside the last slab
    ("euclid", 30, 12, 64, 2, 2, 0.05, 4),
    ("euclid", 50, 10, 128, 2, 1, 0.03, 2),              # 2500 rows <- 100 keys: short key lists, unions of 32-48
]


def _decoder_case(metric, n_out_side, n_in_side, dim, heads, batch, loc, n2, seed=61):
    per = metric != "euclid"
    mo, mi = orc.grid_mesh_2d(n_out_side, not per).reshape(-1, 2), orc.grid_mesh_2d(n_in_side, not per).reshape(-1, 2)
    g = torch.Generator().manual_seed(seed)
    t = dict(values=torch.randn(batch, mi.shape[0], dim, generator=g), lmda=torch.rand(heads, 1, 1, generator=g),
             w1=torch.randn(dim, heads * dim, generator=g) * (2.0 / (heads * dim)) ** 0.5, b1=0.1 * torch.randn(dim, generator=g),
             w2=torch.randn(n2, dim, generator=g) * (2.0 / dim) ** 0.5, b2=0.1 * torch.randn(n2, generator=g))
    d_y = torch.randn(batch, mo.shape[0], n2, generator=g)
    return mo, mi, t, d_y


def _oracle_decoder(metric, batched, mo, mi, t, loc, d_y):
    p = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    ref = orc.mlp(orc.posatt_cross(metric, batched, mo, mi, p["values"], p["lmda"], loc), p["w1"], p["b1"], p["w2"], p["b2"])
    ref.backward(d_y)
    return ref, p


@pytest.mark.parametrize("metric,n_out_side,n_in_side,dim,heads,batch,loc,n2", CASES)
def test_folded_decoder_against_the_oracle(metric, n_out_side, n_in_side, dim, heads, batch, loc, n2):
    """de(up(values)) (pit.py:124-127) with de.mlp1 folded into the values - pit_linear_fwd on the latent points, pit_fold_att_fwd /
    _bwd on the tallest slabs whose unions fit, pit_thin_tail_* - against the oracle's posatt_cross + kaiming_mlp: prediction
    <= 1e-6, d(values) and every weight gradient <= 1e-5, d(lmda) <= 1e-4 (fp32 math mode, exact head scales)."""
    from position_induced_transformer_amd import ops
    mo, mi, t, d_y = _decoder_case(metric, n_out_side, n_in_side, dim, heads, batch, loc, n2)
    ref, p0 = _oracle_decoder(metric, False, mo, mi, t, loc, d_y)
    plan = ops.MeshPlan(metric, mo.cuda(), mi.cuda(), loc, False)
    assert ops.fold_att_supported(plan, heads, dim, batch), "no fold plan for this mesh pair"
    fp = plan.fold_plan()
    assert fp[0].rows in (64, 128, 256) and fp[1] <= 64
    with ops.head_scale_route("host"):
        p1 = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
        y = ops.fold_decoder_apply(p1["values"], p1["lmda"], plan, heads, (p1["w1"], p1["b1"], p1["w2"], p1["b2"]), True)
        y.backward(d_y.cuda())
    torch.cuda.synchronize()
    assert _rel(y, ref) <= 1e-6
    for k in ("values", "w1", "b1", "w2", "b2"):
        assert _rel(p1[k].grad, p0[k].grad) <= 1e-5, (k, _rel(p1[k].grad, p0[k].grad))
    assert float((p1["lmda"].grad.cpu().reshape(-1) - p0["lmda"].grad.reshape(-1)).norm()) <= 1e-4 * float(p0["lmda"].grad.norm())


@pytest.mark.parametrize("metric,n_out_side,n_in_side,dim,heads,batch,loc,n2", CASES)
def test_folded_decoder_in_bf16_mode(metric, n_out_side, n_in_side, dim, heads, batch, loc, n2):
    """The same in the bf16 math mode: tiles rounded to bf16 in LDS, v_mfma_f32_16x16x32_bf16 (the [k][n] images through
    ds_read_b64_tr_b16), z / dz stored as bf16 - within the mode's tolerances against the fp32 oracle (tests/test_gpu_bf16.py)."""
    from position_induced_transformer_amd import ops
    mo, mi, t, d_y = _decoder_case(metric, n_out_side, n_in_side, dim, heads, batch, loc, n2)
    ref, p0 = _oracle_decoder(metric, False, mo, mi, t, loc, d_y)
    plan = ops.MeshPlan(metric, mo.cuda(), mi.cuda(), loc, False)
    with ops.math_mode("bf16"), ops.head_scale_route("host"):
        p1 = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
        y = ops.fold_decoder_apply(p1["values"], p1["lmda"], plan, heads, (p1["w1"], p1["b1"], p1["w2"], p1["b2"]), True)
        y.backward(d_y.cuda())
    torch.cuda.synchronize()
    assert _rel(y, ref) <= 2e-2
    for k in ("values", "w1", "b1", "w2", "b2"):
        assert _rel(p1[k].grad, p0[k].grad) <= 5e-2, (k, _rel(p1[k].grad, p0[k].grad))
    assert float((p1["lmda"].grad.cpu().reshape(-1) - p0["lmda"].grad.reshape(-1)).norm()) <= 5e-2 * float(p0["lmda"].grad.norm())


@pytest.mark.parametrize("bf16", [False, True])
def test_folded_decoder_on_per_sample_meshes_one_head(bf16):
    """NACA's kind of decoder (train_naca.py:79-89: per-sample meshes, one head, hid 128, four output channels): the fold with the
    attention on the candidate-list / union-tile kernels of posatt_apply."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(3)
    b, n_in, n_out, dim, n2, loc = 2, 160, 1500, 128, 4, 0.05
    mi = torch.rand(b, n_in, 2, generator=g)
    mo = torch.rand(b, n_out, 2, generator=g)
    t = dict(values=torch.randn(b, n_in, dim, generator=g), lmda=torch.rand(1, 1, 1, generator=g),
             w1=torch.randn(dim, dim, generator=g) * (2.0 / dim) ** 0.5, b1=0.1 * torch.randn(dim, generator=g),
             w2=torch.randn(n2, dim, generator=g) * (2.0 / dim) ** 0.5, b2=0.1 * torch.randn(n2, generator=g))
    d_y = torch.randn(b, n_out, n2, generator=g)
    ref, p0 = _oracle_decoder("euclid", True, mo, mi, t, loc, d_y)
    plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), loc, False)
    ctxs = (ops.math_mode("bf16"), ops.head_scale_route("host")) if bf16 else (ops.head_scale_route("host"),)
    from contextlib import ExitStack
    with ExitStack() as st:
        for c in ctxs:
            st.enter_context(c)
        p1 = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
        y = ops.fold_decoder_apply(p1["values"], p1["lmda"], plan, 1, (p1["w1"], p1["b1"], p1["w2"], p1["b2"]), False)
        y.backward(d_y.cuda())
    torch.cuda.synchronize()
    # (bf16: ONE layer's d(lmda) - a sum that cancels to a few percent of its terms - from a bf16-stored gradient: 11 % off on this
    # seed with the per-row kernels; the model-level tests judge all layers' d(lmda) as one vector at 5e-2)
    to, tg, tl = (2e-2, 5e-2, 2e-1) if bf16 else (1e-6, 1e-5, 1e-4)
    assert _rel(y, ref) <= to
    for k in ("values", "w1", "b1", "w2", "b2"):
        assert _rel(p1[k].grad, p0[k].grad) <= tg, (k, _rel(p1[k].grad, p0[k].grad))
    assert float((p1["lmda"].grad.cpu().reshape(-1) - p0["lmda"].grad.reshape(-1)).norm()) <= tl * float(p0["lmda"].grad.norm())


def test_fold_plan_picks_the_tallest_slabs_and_refuses_incoherent_meshes():
    """MeshPlan.fold_plan: Vorticity's 64^2 <- 16^2 periodic pair takes 256-row slabs (unions of exactly 64 keys); a randomly
    ordered cloud has unions beyond a tile even at 64 rows and keeps the per-layer path."""
    from position_induced_transformer_amd import ops
    mo, mi = orc.grid_mesh_2d(64, False).reshape(-1, 2), orc.grid_mesh_2d(16, False).reshape(-1, 2)
    plan = ops.MeshPlan("periodic2d", mo.cuda(), mi.cuda(), 0.02, False)
    sp, max_union, _keep, _mc = plan.fold_plan()
    assert (sp.rows, sp.n_slabs, max_union) == (256, 16, 64)
    g = torch.Generator().manual_seed(0)
    cloud_o, cloud_i = torch.rand(4390, 2, generator=g), torch.rand(896, 2, generator=g)
    plan2 = ops.MeshPlan("euclid", cloud_o.cuda(), cloud_i.cuda(), 0.01, False)
    assert plan2.fold_plan() is None
    assert not ops.fold_att_supported(plan2, 1, 256, 4)


def test_models_take_the_folded_decoder_where_it_pays():
    """pit.decoder dispatch: Vorticity (hid 256, two heads, shared meshes) and NACA (hid 128, one head, per-sample meshes) run the
    folded decoder; Elasticity (as many output as latent points) and Darcy b=8 (the fused edge launches) do not."""
    from position_induced_transformer_amd import ops, tasks
    calls = []
    orig = ops.fold_decoder_apply

    def spy(*a, **k):
        calls.append(a[5])
        return orig(*a, **k)
    ops.fold_decoder_apply = spy
    try:
        want = {"vorticity": [True], "naca": [False], "elasticity": [], "darcy": []}
        for name, expect in want.items():
            calls.clear()
            model, sample, meta = tasks.make_task(name, seed=1)
            batch = sample(2)
            with torch.no_grad():
                model(*batch[:3])
            assert calls == expect, (name, calls)
    finally:
        ops.fold_decoder_apply = orig
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- the N > 1 bench line proves itself
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench_child(nproc, extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "5", "--warmup", "2",
           "--full", "--no-extras", "--no-cpu-baseline", "--ddp-sweep"] + extra
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    said = "\n--- child stdout ---\n" + res.stdout[-3000:] + "\n--- child stderr ---\n" + res.stderr[-6000:]
    assert res.returncode == 0, said
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, said
    return json.loads(lines[0]), said


def _check_parity_block(p, said):
    assert "error" not in p, said
    tol = p["tolerance"]
    assert p["rel_l2_out"] <= tol["out"] and p["rel_loss"] <= 1e-5, p
    assert p["rel_l2_weight_grad_worst"] <= tol["weight_grad"], p
    assert p["rel_l2_dlmda_all_layers"] <= tol["dlmda_all_layers"], p


def test_one_rank_bench_line_carries_the_ddp_parity_block_and_the_saturated_point():
    """`torch.distributed.run --nproc-per-node 1 bench.py` (the driver's N > 1 launch with one rank): the record carries
    `parity_ddp` - the all-reduced (RCCL, captured in the hipGraph) flat gradient against the oracle on the global batch rebuilt
    from the ranks' seeds - and the collective saturated-batch scaling point."""
    rec, said = _bench_child(1, ["--sweep-batch", "32"])
    assert rec["config"]["allreduce"]["backend"] == "nccl" and rec["config"]["allreduce"]["captured"] is True
    assert rec["parity_ddp"]["world"] == 1
    _check_parity_block(rec["parity_ddp"], said)
    sweep = rec["batch_sweep_ddp_samples_per_s"]
    assert "error" not in sweep and sweep["32"] > rec["value"], (sweep, rec["value"])


def test_two_ranks_on_one_gpu_bench_line_proves_the_summed_gradient():
    """Two ranks of bench.py sharing this box's one MI355X (backend gloo: the flat gradient is exchanged through the host, outside
    the graph): each runs the HIP step on its own shard (seeds 100 + rank); `parity_ddp` holds the exchanged gradient to the
    oracle's gradient of the 16-sample GLOBAL batch, the summed loss to its loss, rank 0's prediction to its shard's - the
    W-rank == 1-rank check of SURVEY 8(e) on the product path, with W = 2."""
    rec, said = _bench_child(2, ["--backend", "gloo", "--device-index", "0", "--sweep-batch", "16"])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 16
    assert rec["config"]["allreduce"]["backend"] == "gloo" and rec["config"]["allreduce"]["captured"] is False
    assert rec["parity_ddp"]["world"] == 2
    _check_parity_block(rec["parity_ddp"], said)
    assert "error" not in rec["batch_sweep_ddp_samples_per_s"], said


# --------------------------------------------------------------------------- one-launch MLP chains of the bf16 mode (csrc/pit_chain.hip)
@pytest.mark.parametrize("rows,n0,n1", [(5120, 768, 256), (2 * 728, 256, 128), (9720, 768, 256), (1030, 512, 256)])
def test_mlp_chain_against_the_fp64_formula(rows, n0, n1):
    """gelu(kaiming_mlp(x)) (pit.py:21-26 + :121) for hid 128 / 256 on a few thousand rows in the bf16 math mode: pit_mlp_chain_fwd /
    _bwd (one launch per direction, bf16 weight panels through LDS, ds_read_b64_tr_b16 in the backward) against the fp64 formula at
    the mode's tolerances - and against the SAME mode's two-GEMM path, which rounds the same operands (<= 1e-2)."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(rows + n0)
    x = torch.randn(rows, n0, generator=g)
    w1 = torch.randn(n1, n0, generator=g) * (2.0 / n0) ** 0.5
    b1 = 0.1 * torch.randn(n1, generator=g)
    w2 = torch.randn(n1, n1, generator=g) * (2.0 / n1) ** 0.5
    b2 = 0.1 * torch.randn(n1, generator=g)
    dy = torch.randn(rows, n1, generator=g)
    t0 = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    ref = F.gelu(F.linear(F.gelu(F.linear(t0[0], t0[1], t0[2])), t0[3], t0[4]))
    ref.backward(dy.double())
    res = {}
    for chain in (True, False):
        saved = ops.CHAIN_MLP
        ops.CHAIN_MLP = chain
        try:
            with ops.math_mode("bf16"):
                assert ops.chain_mlp_supported(rows, n0, n1, n1, True) == chain
                t1 = [t.cuda().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
                y = ops.mlp_apply(t1[0], t1[1], t1[2], t1[3], t1[4], out_gelu=True)
                y.backward(dy.cuda())
        finally:
            ops.CHAIN_MLP = saved
        torch.cuda.synchronize()
        res[chain] = [y.detach()] + [t.grad for t in t1]
    want = [ref.detach()] + [t.grad for t in t0]
    for i, name in enumerate(("y", "d_x", "d_w1", "d_b1", "d_w2", "d_b2")):
        assert _rel(res[True][i], want[i]) <= (2e-2 if i == 0 else 5e-2), (name, _rel(res[True][i], want[i]))
        assert _rel(res[True][i], res[False][i]) <= 1.5e-2, (name, _rel(res[True][i], res[False][i]))


def test_chain_weights_follow_the_parameters():
    """The chains read cached bf16 copies of the weights: an in-place update of a weight (version counter) and a raw-pointer update
    announced by ops.parameters_changed() (ddp.FlatAdam, a replayed graph) must both reach the next forward."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2048, 256, generator=g).cuda()
    w1 = (torch.randn(128, 256, generator=g) * 0.1).cuda()
    w2 = (torch.randn(128, 128, generator=g) * 0.1).cuda()
    b = torch.zeros(128).cuda()
    with ops.math_mode("bf16"):
        y0 = ops.mlp_apply(x, w1, b, w2, b, out_gelu=True).clone()
        w1.mul_(2.0)                                   # version counter moves
        y1 = ops.mlp_apply(x, w1, b, w2, b, out_gelu=True).clone()
        w2.view(-1).data_ptr()                         # (raw-pointer writers do not touch the counter)
        torch.cuda.synchronize()
        w2.data.copy_(2.0 * w2.data)                   # .data: no version bump
        ops.parameters_changed()
        y2 = ops.mlp_apply(x, w1, b, w2, b, out_gelu=True).clone()
        ref1 = F.gelu(F.linear(F.gelu(F.linear(x, w1, b)), w2 / 2.0, b))
        ref2 = F.gelu(F.linear(F.gelu(F.linear(x, w1, b)), w2, b))
    torch.cuda.synchronize()
    assert _rel(y1, ref1) <= 2e-2 and _rel(y2, ref2) <= 2e-2
    assert _rel(y0, y1) > 0.1 and _rel(y1, y2) > 0.1


def test_fold_attention_backward_is_reproducible_and_matches_the_atomic_form():
    """d(values) of the fold attention: per-slab sums into tiles + a fixed-order reduction per key (ops.FOLD_TILES: taken up to 64 MB of tiles) gives
    the SAME BITS on every pass - the reference's scripts set cudnn.deterministic (pit.py:6) - and agrees with the fp32-atomic form
    to the atomics' summation order; torch.use_deterministic_algorithms keeps the fold path."""
    from position_induced_transformer_amd import ops
    mo, mi, t, d_y = _decoder_case("periodic2d", 64, 16, 256, 2, 3, 0.02, 1)
    plan = ops.MeshPlan("periodic2d", mo.cuda(), mi.cuda(), 0.02, False)
    vw = torch.randn(3, mi.shape[0], 512, generator=torch.Generator().manual_seed(4)).cuda()
    dz = torch.randn(3, mo.shape[0], 256, generator=torch.Generator().manual_seed(5)).cuda()
    lm = t["lmda"].cuda()

    def run():
        v = vw.clone().requires_grad_(True)
        z = ops._FoldAtt.apply(v, lm.reshape(-1), plan, 2, False, None, None, False, False)
        z.backward(dz)
        torch.cuda.synchronize()
        return v.grad.clone()
    a, b = run(), run()
    assert torch.equal(a, b)
    saved = ops.FOLD_TILES
    ops.FOLD_TILES = "0"
    try:
        c = run()
    finally:
        ops.FOLD_TILES = saved
    assert _rel(c, a) <= 1e-6
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert ops.fold_att_supported(plan, 2, 256, 3)
    finally:
        torch.use_deterministic_algorithms(False)


# --------------------------------------------------------------------------- dense self-attention on bf16 MFMA (csrc/pit_satt.hip)
@pytest.mark.parametrize("metric,batched,L,dim,heads,batch", [
    ("euclid", True, 972, 256, 2, 2),            # Elasticity's processor layer (train_elasticity.py:67-75): per-sample clouds
    ("euclid", True, 728, 128, 1, 3),            # NACA's (train_naca.py:79-89)
    ("periodic2d", False, 256, 256, 2, 3),       # Vorticity's: one 16 x 16 periodic mesh for the batch
    ("euclid", True, 300, 128, 2, 2),            # a point count that is no multiple of the 64-row tiles / 32-key steps
    ("periodic1d", False, 256, 128, 1, 2),
    ("euclid", False, 400, 256, 1, 2),           # one head at hid 256 on a batch-free cloud (Cylinder's processor shape)
    ("euclid", True, 2048, 256, 2, 5),           # the largest layer the kernels take; 128-row workgroups in every mode
])
def test_dense_self_attention_on_bf16_mfma_against_the_oracle(metric, batched, L, dim, heads, batch):
    """posatt.forward (pit.py:37-57, locality 1.0) in the bf16 math mode - pit_satt_fwd / _bwd: values rounded once per layer, weights formed
    in registers in the A-fragment layout of v_mfma_f32_16x16x32_bf16, a wavefront per 16 rows x all columns - against the oracle's
    posatt_self at the mode's tolerances; the concat's input columns and their residual gradient are exact."""
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(L + dim)
    if metric == "euclid":
        mesh = torch.rand(batch, L, 2, generator=g) if batched else torch.rand(L, 2, generator=g)
    elif metric == "periodic2d":
        mesh = orc.grid_mesh_2d(16, False).reshape(-1, 2)
    else:
        mesh = orc.line_mesh_1d(L)
    values = torch.randn(batch, L, dim, generator=g)
    lmda = torch.rand(heads, 1, 1, generator=g)
    d_out = torch.randn(batch, L, (1 + heads) * dim, generator=g)
    v0, l0 = values.clone().requires_grad_(True), lmda.clone().requires_grad_(True)
    ref = orc.posatt_self(metric, batched, mesh, v0, l0, 1.0)
    ref.backward(d_out)
    plan = ops.MeshPlan(metric, mesh.cuda(), mesh.cuda(), 1.0, True)
    calls = {"n": 0}
    L_ = ops._lib.lib()
    real = L_.pit_satt_fwd

    def counted(*a):
        calls["n"] += 1
        return real(*a)

    saved = ops.SATT
    L_.pit_satt_fwd = counted
    try:
        with ops.math_mode("bf16"), ops.head_scale_route("host"):
            assert L_.pit_satt_supported(L, heads, dim, batch, plan.mesh_batch)
            ops.SATT = "1"                       # ("auto" keeps these kernels for the shapes where they measured faster: ops._satt_pays)
            v1, l1 = values.cuda().requires_grad_(True), lmda.cuda().requires_grad_(True)
            out = ops.posatt_apply(v1, l1, plan, heads, concat=True)
            out.backward(d_out.cuda())
            assert calls["n"] == 1
            # d(values) on the forward's weight tiles (the default) and with the weights formed again: the same rounded weights
            tiles_were = ops.SATT_TILES
            ops.SATT_TILES = False
            try:
                v3, l3 = values.cuda().requires_grad_(True), lmda.cuda().requires_grad_(True)
                out3 = ops.posatt_apply(v3, l3, plan, heads, concat=True)
                out3.backward(d_out.cuda())
            finally:
                ops.SATT_TILES = tiles_were
            assert calls["n"] == 2 and tiles_were
            # (d(scale) forms its operand from the tile's rounded weight x (m - mbar): rounded twice, not once - 1e-4 at Elasticity's
            # layer, 6e-3 on 2048 random points where d(lmda) is a small difference of large sums; the bound against the oracle is 5e-2)
            assert torch.equal(out3, out) and _rel(v3.grad, v1.grad) <= 1e-6 and _rel(l3.grad, l1.grad) <= 2e-2
            # the same layer on the register-rounding kernels of the earlier rounds: both are the bf16 mode
            ops.SATT = "0"
            v2, l2 = values.cuda().requires_grad_(True), lmda.cuda().requires_grad_(True)
            out2 = ops.posatt_apply(v2, l2, plan, heads, concat=True)
            out2.backward(d_out.cuda())
            assert calls["n"] == 2
            ops.SATT = "auto"
            assert ops._satt_pays(972, 2, 256) and ops._satt_pays(728, 1, 128) and ops._satt_pays(256, 2, 256) and not ops._satt_pays(128, 2, 256)
    finally:
        ops.SATT = saved
        L_.pit_satt_fwd = real
    torch.cuda.synchronize()
    assert torch.equal(out[..., :dim].cpu(), values)
    assert _rel(out[..., dim:], ref[..., dim:]) <= 2e-2
    assert _rel(v1.grad, v0.grad) <= 2e-2
    assert float((l1.grad.cpu().reshape(-1) - l0.grad.reshape(-1)).norm()) <= 5e-2 * float(l0.grad.norm())
    assert _rel(out[..., dim:], out2[..., dim:]) <= 1e-2 and _rel(v1.grad, v2.grad) <= 1.5e-2


def test_mlp_chains_write_the_self_attention_operands_and_the_prep_launches_go():
    """Two processor blocks' worth of pit.py:114-122 in the bf16 mode - kaiming_mlp -> posatt.forward -> kaiming_mlp: the chain in front
    writes bf16(y) beside y (pit_mlp_chain_fwd's y16 = pit_satt_fwd's x16), the chain behind writes G16 = bf16(d_x_h / rowsum_h) beside d_x
    (pit_mlp_chain_bwd's g16 = pit_satt_bwd's) - the same bits the two prep launches would have produced, so results are IDENTICAL with
    the hand-offs on and off; and the hand-offs are really taken (counted on the library entry points' flags)."""
    from position_induced_transformer_amd import ops
    torch.manual_seed(11)
    b, L, d, H = 3, 640, 128, 2
    mesh = torch.rand(b, L, 2).cuda()
    plan = ops.MeshPlan("euclid", mesh, mesh, 1.0, True)
    x0 = torch.randn(b, L, 3 * d).cuda()
    lm = torch.rand(H, 1, 1).cuda()
    ws = [(torch.randn(d, 3 * d).cuda() * 0.05, torch.randn(d).cuda() * 0.1, torch.randn(d, d).cuda() * 0.08, torch.randn(d).cuda() * 0.1) for _ in range(2)]
    d_out = torch.randn(b, L, d).cuda()
    L_ = ops._lib.lib()
    real_f, real_b = L_.pit_satt_fwd, L_.pit_satt_bwd
    seen = {"x16_ready": [], "g16_ready": []}

    def fwd(*a):
        seen["x16_ready"].append(int(a[-2]))
        return real_f(*a)

    def bwd(*a):
        seen["g16_ready"].append(int(a[-3]))
        return real_b(*a)

    def run(fuse):
        saved = ops.SATT, ops.SATT_FUSE_PREP
        ops.SATT, ops.SATT_FUSE_PREP = "1", fuse
        try:
            with ops.math_mode("bf16"), ops.head_scale_route("host"):
                x = x0.clone().requires_grad_(True)
                l1 = lm.clone().requires_grad_(True)
                p = [tuple(t.clone().requires_grad_(True) for t in w) for w in ws]
                y = ops.mlp_apply(x, *p[0], out_gelu=True, concat_heads=H)
                a = ops.posatt_apply(y, l1, plan, H, concat=True)
                z = ops.mlp_apply(a, *p[1], out_gelu=True)
                z.backward(d_out)
                torch.cuda.synchronize()
                return [z.detach(), x.grad, l1.grad] + [t.grad for w in p for t in w]
        finally:
            ops.SATT, ops.SATT_FUSE_PREP = saved

    L_.pit_satt_fwd, L_.pit_satt_bwd = fwd, bwd
    try:
        on = run(True)
        assert seen == {"x16_ready": [1], "g16_ready": [1]}
        off = run(False)
        assert seen == {"x16_ready": [1, 0], "g16_ready": [1, 0]}
    finally:
        L_.pit_satt_fwd, L_.pit_satt_bwd = real_f, real_b
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])             # prediction, d(input)
    for u, v in zip(on[2:], off[2:]):                                            # (d(lmda), weight gradients: sums of atomic adds)
        assert _rel(u, v) <= 1e-5
