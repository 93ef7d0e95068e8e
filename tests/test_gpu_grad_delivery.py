"""GPU: where the fused autograd nodes of ops.py deliver d(lmda) and an MLP's weight gradients - returned to autograd, accumulated
in place into the parameter's .grad now, or in place with d(lmda) finished by the pass's one deferred launch - at every backward
site that decides it: _PosAtt (candidate lists, dense self-attention on bf16 MFMA, union tiles), _PosAttPre, _Processor, _Decoder,
_FoldAtt, _Encoder and the three ways _Mlp.backward reaches its weight-gradient reductions in the fp32 mode.

Per case the same forward + backward runs
  (a) with fresh parameters whose .grad is None: every gradient is returned to autograd,
  (b) with the parameters registered in a ddp.FlatGradients (in place) and ops.DEFER_HEAD_FINISH off,
  (c) in place and deferred,
  (d) as (c), two passes without zeroing in between.
(b) and (c) must equal (a), (d) must equal 2 x (a); nothing may be left in ops._PENDING_HEADS / ops._PENDING_DW; the autograd graph
must hold the node the case is about and the library entry of its backward must have run (a support predicate that quietly sends
the shape elsewhere fails the case); pit_posatt_dhead_finish must have been launched as often as the delivery mode says.

Bounds, from tests/test_gpu_models.py::test_deferred_head_finish_matches_per_layer_finish: d(lmda) between modes 1e-6 + 5e-7,
weight gradients between modes 5e-7 (both rel-L2 against (a)), the doubled pass 1e-5.

Shapes: the lower edges of the support predicates - the 20 x 20 <-> 16 x 16 jittered pair of test_gpu_fused_envelope (PAIRS / UNIONS)
for the edge launches, the fold and the candidate-list layers, 256 latent points x batch 2 x two blocks for the fused processor, 64
points x hid 256 for the bf16 dense self-attention, the smallest shapes pit_posatt_pre_supported takes for _PosAttPre, and
the two at which its rows launch takes two and four row tiles per workgroup."""
import contextlib

import pytest
import torch

import golden_io as gio
from test_gpu_fused_envelope import UNIONS, _model, _processor_parts, lattice
from test_gpu_mesh_grad import LaunchLog

pytestmark = pytest.mark.gpu

TOL_HEAD, TOL_WEIGHT, TOL_TWICE = 1e-6 + 5e-7, 5e-7, 1e-5
MODES = ("returned", "inplace", "deferred")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _param(t):
    return torch.nn.Parameter(t.cuda())


def _head(heads, g, is_scale):
    """An (H, 1, 1) lmda, or the head scale c itself (1..7) when the layer takes its head as the scale."""
    u = torch.rand(heads, 1, 1, generator=g)
    return _param(1.0 + 6.0 * u if is_scale else u)


def _mlp(n0, n1, n2, g, tag=""):
    return {f"w1{tag}": _param(torch.randn(n1, n0, generator=g) * (2.0 / n0) ** 0.5), f"b1{tag}": _param(0.1 * torch.randn(n1, generator=g)),
            f"w2{tag}": _param(torch.randn(n2, n1, generator=g) * (2.0 / n1) ** 0.5), f"b2{tag}": _param(0.1 * torch.randn(n2, generator=g))}


def _pair():
    """(mesh A (400, 2), mesh B (256, 2), locality) of UNIONS["48-slots-full"] (= PAIRS["2d"]): jittered 20 x 20 and 16 x 16 lattices."""
    sa, seed_a, sb, seed_b, loc, _union, _fused = UNIONS["48-slots-full"]
    return lattice(sa, seed_a).cuda(), lattice(sb, seed_b).cuda(), loc


class Case:
    """params: name -> Parameter (fresh objects, the same values on every build); forward() -> the output; d_out: its gradient;
    node: class name of the autograd node; entries(mode) -> {library entry: launches per pass} that must hold; finishes: launches of
    pit_posatt_dhead_finish per pass in modes (a), (b), (c); bf16 / satt: the math mode and ops.SATT the case runs under."""

    def __init__(self, params, forward, d_out, node, entries, finishes, bf16=False, satt=False):
        self.params, self.forward, self.d_out, self.node, self.entries, self.finishes = params, forward, d_out.cuda(), node, entries, finishes
        self.bf16, self.satt = bf16, satt


def _always(**counts):
    return lambda mode: counts


# --------------------------------------------------------------------------- _PosAtt
def posatt_lists():
    """Masked cross attention on candidate lists, two heads, batch 2: the generic launch finishes d(lmda) itself unless deferred."""
    from position_induced_transformer_amd import ops
    a, b, loc = _pair()
    g = _gen(11)
    plan = ops.MeshPlan("euclid", a, b, loc, False)
    assert plan.nbr_idx is not None, "no candidate lists"
    lm = _head(2, g, False)
    x = torch.randn(2, 256, 32, generator=g).cuda().requires_grad_(True)
    return Case({"lmda": lm}, lambda: ops.posatt_apply(x, lm, plan, 2, concat=False), torch.randn(2, 400, 64, generator=g),
                "_PosAttBackward", _always(pit_posatt_bwd=1, pit_satt_bwd=0, pit_union_att_bwd=0), (0, 0, 1))


def posatt_satt():
    """Dense self-attention on bf16 MFMA (ops.SATT forced on, bf16 mode): 64 points, hid 256, two heads, batch 2."""
    from position_induced_transformer_amd import ops
    g = _gen(12)
    mesh = lattice((8, 8), 12).cuda()
    plan = ops.MeshPlan("euclid", mesh, mesh, 1.0, True)
    assert ops._lib.lib().pit_satt_supported(64, 2, 256, 2, 1)
    lm = _head(2, g, False)
    x = torch.randn(2, 64, 256, generator=g).cuda().requires_grad_(True)
    return Case({"lmda": lm}, lambda: ops.posatt_apply(x, lm, plan, 2, concat=True), torch.randn(2, 64, 768, generator=g),
                "_PosAttBackward", _always(pit_satt_bwd=1, pit_posatt_bwd=0), (1, 1, 1), bf16=True, satt=True)


def posatt_union():
    """Masked cross attention on the union-tile contraction (hid 128: below it a layer keeps the candidate-list kernels)."""
    from position_induced_transformer_amd import ops
    a, b, loc = _pair()
    g = _gen(13)
    plan = ops.MeshPlan("euclid", a, b, loc, False)
    lm = _head(2, g, False)
    x = torch.randn(2, 256, 128, generator=g).cuda().requires_grad_(True)
    assert ops._union_att_ok(plan, 2, 128, 2, x.detach()), "the union-tile launches refuse this layer"
    return Case({"lmda": lm}, lambda: ops.posatt_apply(x, lm, plan, 2, concat=False), torch.randn(2, 400, 256, generator=g),
                "_PosAttBackward", _always(pit_union_att_bwd=1, pit_posatt_bwd=0), (1, 1, 1))


# --------------------------------------------------------------------------- _PosAttPre
def _pre(shape, heads, dim, batch):
    from position_induced_transformer_amd import ops
    g = _gen(20 + heads)
    mesh = lattice(shape, 20 + heads).cuda()
    n = mesh.shape[0]
    assert ops.pre_weights_supported(n, heads, dim, batch, 2), "pit_posatt_pre_supported refuses this shape"
    plan = ops.MeshPlan("euclid", mesh, mesh, 1.0, True)
    lm = _head(heads, g, False)
    x = torch.randn(batch, n, dim, generator=g).cuda().requires_grad_(True)

    def forward():
        return ops.posatt_pre_apply(x, lm, ops.block_weights(plan, [lm], heads, True), 0, heads)
    return Case({"lmda": lm}, forward, torch.randn(batch, n, (1 + heads) * dim, generator=g), "_PosAttPreBackward",
                _always(pit_posatt_pre_bwd=1), (1, 1, 1))


def pre_two_heads():
    """The smallest two-head shape pit_posatt_pre_supported takes: 768 points, hid 256, batch 4 (batch 2 is below its regime)."""
    return _pre((24, 32), 2, 256, 4)


def pre_one_head():
    """One head: 1024 points, hid 128, batch 8."""
    return _pre((32, 32), 1, 128, 8)


def pre_rt2():
    """Two 32-row tiles per workgroup (the two cases above run one): 1024 points, two heads, hid 256, batch 8 = 2048 columns - the
    regime rule (csrc/pit_posatt.hip: rows_tiles_regime) gives rt = 2 with 8 column tiles per workgroup."""
    return _pre((32, 32), 2, 256, 8)


def pre_rt4():
    """Four row tiles per workgroup: the same layer at batch 16 = 4096 columns - rt = 4, 8 column tiles per workgroup."""
    return _pre((32, 32), 2, 256, 16)


# --------------------------------------------------------------------------- _Processor
def processor():
    """Two fused blocks on 256 latent points, two heads, batch 2 (512 rows): d(lmda) of both blocks from ONE finishing launch."""
    from position_induced_transformer_amd import ops
    mesh = lattice((16, 16), 30)
    model = _model("euclid", 2, 1, 1, 64, 2, 2, mesh, 0.02, 31)
    assert ops.block_fusion_supported(256, 2, 64, 2, 2)
    lmdas, mlps = _processor_parts(model)
    plan = model.conv[0]._plan(model.mesh_ltt, model.mesh_ltt, True)
    g = _gen(32)
    x = torch.randn(2, 256, 64, generator=g).cuda().requires_grad_(True)
    params = {f"lmda{i}": p for i, p in enumerate(lmdas)}
    for i, m in enumerate(mlps):
        params.update({f"{k}_{i}": t for k, t in zip(("w1", "b1", "w2", "b2"), m)})
    return Case(params, lambda: ops.processor_apply(x, plan, 2, lmdas, mlps), torch.randn(2, 256, 64, generator=g),
                "_ProcessorBackward", _always(pit_block_bwd=2), (1, 1, 1))


# --------------------------------------------------------------------------- _Decoder, _FoldAtt, _Encoder
def _decoder(is_scale):
    from position_induced_transformer_amd import ops
    a, b, loc = _pair()
    g = _gen(40)
    plan = ops.MeshPlan("euclid", a, b, loc, False)
    assert ops.edge_fusion_supported(plan, 2, 32, 2, True), "the fused decoder refuses this layer"
    params = {"lmda": _head(2, g, is_scale), **_mlp(64, 32, 1, g)}
    x = torch.randn(2, 256, 32, generator=g).cuda().requires_grad_(True)
    mlp = tuple(params[k] for k in ("w1", "b1", "w2", "b2"))
    # (d(b2) is ONE number, the sum of d_out over 800 rows by fp32 atomic adds: with a zero-mean d_out it cancels to a thirtieth of its
    # terms and moves by 2 ulp = 2.8e-7 from run to run of one mode; around a mean of 1 the sum is well conditioned)
    d_out = 1.0 + 0.5 * torch.randn(2, 400, 1, generator=g)
    return Case(params, lambda: ops.decoder_apply(x, params["lmda"], plan, 2, mlp, head_is_scale=is_scale),
                d_out, "_DecoderBackward", _always(pit_decoder_bwd=1), (1, 1, 1))


def decoder_lmda():
    """The fused decoder (two heads, hid 32, batch 2, one output channel), head = lmda."""
    return _decoder(False)


def decoder_scale():
    """The same with the head handed over as the scale c."""
    return _decoder(True)


def _fold(is_scale):
    from position_induced_transformer_amd import ops
    sa, seed_a, sb, seed_b, loc, _union, _fused = UNIONS["32-slots-full"]
    a, b = lattice(sa, seed_a).cuda(), lattice(sb, seed_b).cuda()
    g = _gen(50)
    plan = ops.MeshPlan("euclid", a, b, loc, False)
    assert ops.fold_att_supported(plan, 2, 64, 2), "no fold plan for this mesh pair"
    lm = _head(2, g, is_scale)
    vw = torch.randn(2, 256, 128, generator=g).cuda().requires_grad_(True)
    return Case({"lmda": lm}, lambda: ops._FoldAtt.apply(vw, lm.reshape(-1), plan, 2, is_scale, lm, None, False, True),
                torch.randn(2, 1024, 64, generator=g), "_FoldAttBackward", _always(pit_fold_att_bwd=1), (1, 1, 1))


def fold_lmda():
    """The fold attention (1024 <- 256 points, two heads, hid 64, batch 2), head = lmda."""
    return _fold(False)


def fold_scale():
    return _fold(True)


def _encoder(heads, is_scale):
    from position_induced_transformer_amd import ops
    a, b, loc = _pair()
    g = _gen(60 + heads)
    plan = ops.MeshPlan("euclid", b, a, loc, False)                     # 256 latent points <- 400 input points
    assert ops.edge_fusion_supported(plan, heads, 32, 2, False), "the fused encoder refuses this layer"
    params = {"lmda": _head(heads, g, is_scale), **_mlp(heads * 3, 32, 32, g)}
    x = torch.randn(2, 400, 3, generator=g).cuda()
    mlp = tuple(params[k] for k in ("w1", "b1", "w2", "b2"))
    return Case(params, lambda: ops.encoder_apply(x, params["lmda"], plan, heads, mlp, head_is_scale=is_scale),
                torch.randn(2, 256, 32, generator=g), "_EncoderBackward", _always(pit_encoder_bwd=1), (1, 1, 1))


def encoder_lmda():
    """The fused encoder (two heads, hid 32, batch 2, three input channels), head = lmda."""
    return _encoder(2, False)


def encoder_scale():
    return _encoder(2, True)


def encoder_one_head():
    return _encoder(1, False)


# --------------------------------------------------------------------------- _Mlp: the fp32 mode's ways to the weight-gradient reductions
def _mlp_entries(split):
    """In place the data path runs alone (pit_mlp_bwd_data) and the reductions are postponed; returned gradients take the one call."""
    def entries(mode):
        if split and mode != "returned":
            return {"pit_mlp_bwd_data": 1, "pit_mlp_bwd": 0}
        return {"pit_mlp_bwd_data": 0, "pit_mlp_bwd": 1}
    return entries


def mlp_small_rider():
    """A small-regime MLP (800 rows, 64 -> 32 -> 32, trailing gelu) behind a candidate-list attention layer: in place its reductions are
    postponed (MLP_PARAMS_RIDER) and ride in that layer's backward launch."""
    from position_induced_transformer_amd import ops
    a, b, loc = _pair()
    g = _gen(70)
    plan = ops.MeshPlan("euclid", a, b, loc, False)
    assert ops._dw_deferrable(800, 64, 32, 32, 1, 32)
    params = {"lmda": _head(2, g, False), **_mlp(64, 32, 32, g)}
    x = torch.randn(2, 256, 32, generator=g).cuda().requires_grad_(True)

    def forward():
        y = ops.posatt_apply(x, params["lmda"], plan, 2, concat=False)
        return ops.mlp_apply(y, params["w1"], params["b1"], params["w2"], params["b2"], out_gelu=True)
    return Case(params, forward, torch.randn(2, 400, 32, generator=g), "_MlpBackward", _mlp_entries(True), (0, 0, 1))


def mlp_wide_rider():
    """The large regime behind a dense self-attention layer (4096 rows, 256 -> 128 -> 128: not deferrable as a small job): in place the
    reductions ride in the attention's merged backward launch (WIDE_DW_RIDER)."""
    from position_induced_transformer_amd import ops
    g = _gen(71)
    mesh = lattice((16, 32), 71).cuda()
    plan = ops.MeshPlan("euclid", mesh, mesh, 1.0, True)
    assert not ops._dw_deferrable(4096, 256, 128, 128, 1, 128)
    params = {"lmda": _head(1, g, False), **_mlp(256, 128, 128, g)}
    x = torch.randn(8, 512, 128, generator=g).cuda().requires_grad_(True)

    def forward():
        y = ops.posatt_apply(x, params["lmda"], plan, 1, concat=True)
        assert getattr(y, "_pit_dense_att", False)
        return ops.mlp_apply(y, params["w1"], params["b1"], params["w2"], params["b2"], out_gelu=True)
    return Case(params, forward, torch.randn(8, 512, 128, generator=g), "_MlpBackward", _mlp_entries(True), (0, 0, 1))


def mlp_one_call():
    """Neither: 100 rows, 7 -> 5 -> 3 - the one pit_mlp_bwd call, accumulating in place or into fresh tensors."""
    from position_induced_transformer_amd import ops
    g = _gen(72)
    assert not ops._dw_deferrable(100, 7, 5, 3, 0, 3)
    params = _mlp(7, 5, 3, g)
    x = torch.randn(2, 50, 7, generator=g).cuda().requires_grad_(True)
    return Case(params, lambda: ops.mlp_apply(x, params["w1"], params["b1"], params["w2"], params["b2"]),
                torch.randn(2, 50, 3, generator=g), "_MlpBackward", _mlp_entries(False), (0, 0, 0))


CASES = [posatt_lists, posatt_satt, posatt_union, pre_two_heads, pre_one_head, pre_rt2, pre_rt4, processor, decoder_lmda, decoder_scale, fold_lmda,
         fold_scale, encoder_lmda, encoder_scale, encoder_one_head, mlp_small_rider, mlp_wide_rider, mlp_one_call]


# --------------------------------------------------------------------------- the harness
def _nodes(out):
    names, seen, stack = set(), set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(n for n, _ in fn.next_functions)
    return names


def deliver(build, mode, monkeypatch, passes=1):
    """Gradients of every parameter of a freshly built case after ``passes`` forward + backward passes in delivery mode ``mode``."""
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd.ddp import FlatGradients
    case = build()
    assert all(p.grad is None for p in case.params.values())
    flat = FlatGradients(case.params.values()) if mode != "returned" else None
    views = {k: p.grad.data_ptr() for k, p in case.params.items()} if flat is not None else {}
    with contextlib.ExitStack() as st:
        st.enter_context(monkeypatch.context()).setattr(ops, "DEFER_HEAD_FINISH", mode == "deferred")
        if case.satt:
            st.enter_context(monkeypatch.context()).setattr(ops, "SATT", "1")
        if case.bf16:
            st.enter_context(ops.math_mode("bf16"))
        log = LaunchLog(st.enter_context(monkeypatch.context()))
        for _ in range(passes):
            out = case.forward()
            assert case.node in _nodes(out), f"{case.node} is not in the graph: {sorted(_nodes(out))}"
            out.backward(case.d_out)
        torch.cuda.synchronize()
    assert not ops._PENDING_HEADS, "deferred d(lmda) finishes left pending"
    assert all(v is None for v in ops._PENDING_DW.values()), "a postponed weight-gradient job was left pending"
    for name, want in case.entries(mode).items():
        assert log.count(name) == want * passes, f"{mode}: {name} ran {log.count(name)} times, expected {want * passes}"
    want = case.finishes[MODES.index(mode)] * passes
    assert log.count("pit_posatt_dhead_finish") == want, f"{mode}: {log.count('pit_posatt_dhead_finish')} finishing launches, expected {want}"
    for k, p in case.params.items():
        assert p.grad is not None, f"{mode}: no gradient for {k}"
        if flat is not None:
            assert p.grad.data_ptr() == views[k], f"{mode}: {k}.grad left the flat buffer"
    return {k: p.grad.detach().double().cpu().numpy().copy() for k, p in case.params.items()}


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_gradient_delivery_modes_agree(build, monkeypatch):
    """(b) in place and (c) in place + deferred give the gradients (a) returns to autograd; two deferred passes give twice them."""
    ref = deliver(build, "returned", monkeypatch)
    worst = []
    for mode in ("inplace", "deferred"):
        got = deliver(build, mode, monkeypatch)
        for k in ref:
            err, tol = gio.rel_l2(ref[k], got[k]), (TOL_HEAD if k.startswith("lmda") else TOL_WEIGHT)
            print(f"{build.__name__} {mode} {k}: {err:.3e} (bound {tol:.1e})")
            if err > tol:
                worst.append((mode, k, err))
    twice = deliver(build, "deferred", monkeypatch, passes=2)
    for k in ref:
        err = gio.rel_l2(2.0 * ref[k], twice[k])
        print(f"{build.__name__} twice {k}: {err:.3e} (bound {TOL_TWICE:.1e})")
        if err > TOL_TWICE:
            worst.append(("twice", k, err))
    assert not worst, worst
