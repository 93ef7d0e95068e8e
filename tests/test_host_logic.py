"""CPU: host logic around the HIP path that needs no device - the torch.compile boundary, the
import-time behaviour of pit.py:1-11, exception safety of the deferred d(lmda) finish, the flat
gradient buffer surviving ``optimizer.zero_grad()``, the per-thread math mode / head-scale route."""
import os
import subprocess
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- torch.compile boundary
def test_task_forward_is_opaque_to_dynamo_and_wrapper_keeps_orig_mod_keys():
    """train_darcy.py:112 `model = torch.compile(model)` and :150 `model.state_dict()`: the wrapper
    must carry the `_orig_mod.` keys and calling it must reach OUR operators (which refuse CPU
    tensors with their own message), not fail inside dynamo."""
    from position_induced_transformer_amd import pit as P, tasks
    model, _, _ = tasks.make_task("darcy", device="cpu")
    assert getattr(type(model).forward, "_pit_eager", False)
    compiled = torch.compile(model)
    keys = list(compiled.state_dict().keys())
    assert keys and all(k.startswith("_orig_mod.") for k in keys)
    assert [k[len("_orig_mod."):] for k in keys] == list(model.state_dict().keys())
    with pytest.raises(RuntimeError, match="HIP device only"):
        compiled(torch.zeros(43, 43, 2), torch.zeros(2, 43, 43, 1), torch.zeros(43, 43, 2))
    # torch._dynamo.disable(model) of train_darcy.py:152 is accepted on the compiled wrapper as well
    again = torch._dynamo.disable(compiled)
    with pytest.raises(RuntimeError, match="HIP device only"):
        again(torch.zeros(43, 43, 2), torch.zeros(2, 43, 43, 1), torch.zeros(43, 43, 2))

    class script_model(P.pit_fixed):              # a class written the way the scripts write theirs
        def forward(self, mesh_in, func_in, mesh_out):
            return self.encoder(mesh_in, func_in, self.mesh_ltt)
    assert getattr(script_model.forward, "_pit_eager", False)


def test_operator_entry_points_are_dynamo_disabled():
    from position_induced_transformer_amd import ops
    for fn in (ops.posatt_apply, ops.mlp_apply, ops.rel_lp_loss, ops.instance_norm_points, ops.rel_max_norm):
        assert getattr(fn, "_torchdynamo_disable", False), fn


def test_reference_checkpoint_through_compile_roundtrip(tmp_path):
    """A checkpoint written as the scripts write it (state_dict of the torch.compile wrapper,
    train_darcy.py:150) loads back into a fresh model."""
    from position_induced_transformer_amd import tasks, utils
    model, _, _ = tasks.make_task("darcy", device="cpu", seed=3)
    path = tmp_path / "model.pth"
    torch.save({"model_state": torch.compile(model).state_dict()}, path)
    fresh, _, _ = tasks.make_task("darcy", device="cpu", seed=4)
    utils.load_reference_checkpoint(fresh, str(path))
    for (k, a), (_, b) in zip(model.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), k


# --------------------------------------------------------------------------- import-time behaviour
def _import_probe(env_extra):
    code = ("import torch, numpy as np; torch.manual_seed(1234); np.random.seed(99); "
            "import position_induced_transformer_amd.pit as P; "
            "print(torch.initial_seed(), int(np.random.get_state()[1][0]), torch.get_float32_matmul_precision())")
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    return int(out[0]), int(out[1]), out[2]


def test_import_reproduces_the_reference_side_effects_with_opt_out():
    """pit.py:2-10 seeds torch / numpy with 0 and sets the matmul precision at import; scripts that
    never seed rely on it.  Reproduced by default, switched off by PIT_IMPORT_SIDE_EFFECTS=0."""
    seed, np0, prec = _import_probe({})
    assert seed == 0 and prec == "high"
    import numpy as np
    np.random.seed(0)
    assert np0 == int(np.random.get_state()[1][0])
    seed, _, _ = _import_probe({"PIT_IMPORT_SIDE_EFFECTS": "0"})
    assert seed == 1234


# --------------------------------------------------------------------------- deferred finish, exception safety
def test_deferred_head_finish_survives_a_backward_pass_that_raised(monkeypatch):
    """autograd skips end-of-pass callbacks when a backward raises.  The next pass must
    still queue its flush, must not drain the aborted pass's entries, and must have zeroed the
    accumulators those entries point at."""
    from position_induced_transformer_amd import ops
    flushed = []

    def fake_flush(task):
        flushed.append([p[0] for p in ops._PENDING_HEADS.pop(task)])
    monkeypatch.setattr(ops, "_flush_head_finishes", fake_flush)
    ops._PENDING_HEADS.clear()

    class Layer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, ws, boom):
            ctx.ws, ctx.boom = ws, boom
            return x * 2

        @staticmethod
        def backward(ctx, g):
            ctx.ws += 1.0                                 # "partial sums" of this pass
            ops._defer_head_finish(ctx.ws, None, None, None, 1, 0)
            if ctx.boom:
                raise RuntimeError("boom")
            return g * 2, None, None

    x = torch.ones(3, requires_grad=True)
    ws_a, ws_b = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="boom"):
        Layer.apply(Layer.apply(x, ws_a, False), ws_a, True).sum().backward()
    assert flushed == [] and len(ops._PENDING_HEADS) >= 1         # the callback never ran: entries are stale
    Layer.apply(x, ws_b, False).sum().backward()                    # a healthy pass on OTHER accumulators (another model)
    assert len(flushed) == 1 and len(flushed[0]) == 1 and flushed[0][0] is ws_b
    assert float(ws_a.abs().sum()) > 0.0 and len(ops._PENDING_HEADS) == 1   # ... does not touch the aborted pass's entries
    Layer.apply(x, ws_a, False).sum().backward()                    # the next pass over the SAME accumulators does:
    assert len(flushed) == 2 and len(flushed[1]) == 1 and flushed[1][0] is ws_a
    assert float(ws_a.abs().sum()) == 0.0                            # the aborted pass's partial sums were cleared
    assert ops._PENDING_HEADS == {}
    Layer.apply(x, ws_b, False).sum().backward()                    # and the pass after that is normal again
    assert len(flushed) == 3


# --------------------------------------------------------------------------- flat gradients vs zero_grad()
def test_flat_gradients_reattach_after_optimizer_zero_grad():
    """`optimizer.zero_grad()` (set_to_none=True) drops the views into the flat buffer;
    all_reduce()/attach() must copy the fresh gradients back and re-point .grad, every step."""
    from position_induced_transformer_amd.ddp import FlatGradients
    torch.manual_seed(0)
    lin = torch.nn.Linear(5, 3)
    flat = FlatGradients(lin.parameters())
    opt = torch.optim.SGD(lin.parameters(), lr=0.1)
    for step in range(3):
        opt.zero_grad()                                   # .grad -> None
        x = torch.randn(4, 5)
        lin(x).pow(2).sum().backward()                    # autograd allocates fresh grads outside `flat`
        expect = torch.cat([p.grad.reshape(-1).clone() for p in lin.parameters()])
        assert flat.attach() == 2
        assert torch.equal(flat.dense(), expect), step
        for p, v in zip(flat.params, flat._views):
            assert p.grad.data_ptr() == v.data_ptr()
        assert flat.attach() == 0
        opt.step()
    flat.zero_()
    assert float(flat.flat.abs().sum()) == 0.0 and all(p.grad is not None for p in lin.parameters())


# --------------------------------------------------------------------------- per-thread modes
def test_math_mode_and_head_scale_route_are_per_thread_host_state():
    from position_induced_transformer_amd import ops
    assert ops.get_math_mode() == "fp32" and ops.get_head_scale_route() == "device"
    seen = {}

    def worker():
        seen["before"] = (ops.get_math_mode(), ops.get_head_scale_route())
        ops.set_math_mode("bf16")
        ops.set_head_scale_route("host")
        seen["after"] = (ops.get_math_mode(), ops.get_head_scale_route())
    with ops.math_mode("bf16"), ops.head_scale_route("host"):
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        assert (ops.get_math_mode(), ops.get_head_scale_route()) == ("bf16", "host")
    assert seen["before"] == ("fp32", "device") and seen["after"] == ("bf16", "host")
    assert (ops.get_math_mode(), ops.get_head_scale_route()) == ("fp32", "device")
    with pytest.raises(ValueError):
        ops.set_head_scale_route("gpu")


def test_inplace_gradient_slots_are_opt_in():
    """kernels write into .grad in place only for parameters FlatGradients registered, while
    the registered view is still attached and no hooks sit on the parameter."""
    from position_induced_transformer_amd import ops
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.zeros(4)
    assert ops._grad_slot(p) is None                     # an existing .grad alone is not consent
    ops.mark_inplace_grad(p, p.grad)
    # (CPU tensors never qualify: the check is for device fp32 buffers)
    assert ops._grad_slot(p) is None


def test_satt_handoffs_are_refused_once_the_tensor_changed_in_place():
    """The bf16 operands the MLP chains write for a dense self-attention layer (y16 beside y, G16 beside d_x) are taken only while
    the tensor they were formed from is unchanged: an in-place edit of y, or a gradient accumulated into / scaled in d_x's buffer
    (same address), sends the layer back to its prep launch."""
    from position_induced_transformer_amd import ops
    y = torch.zeros(2, 3, 4)
    x16 = torch.zeros(6, 4, dtype=torch.bfloat16)
    y._pit_x16, y._pit_x16_version = x16, y._version
    assert ops._handoff_x16(y) is x16
    y.mul_(2.0)
    assert ops._handoff_x16(y) is None
    assert ops._handoff_x16(torch.zeros(2, 3, 4)) is None
    y2 = torch.zeros(2, 3, 4)
    y2._pit_x16 = x16                                    # (no recorded version: not trusted)
    assert ops._handoff_x16(y2) is None

    d_x = torch.zeros(6, 12)
    g16 = torch.zeros(2, 2, 3, 4, dtype=torch.bfloat16)
    lk = {"g16": g16, "dx_ptr": d_x.data_ptr(), "dx_version": d_x._version}
    d_out = d_x.reshape(2, 3, 12)                        # (what _Mlp.backward returns: a view, one version counter)
    assert ops._handoff_g16_ready(lk, d_out, (2, 2, 3, 4))
    assert not ops._handoff_g16_ready(lk, d_out, (2, 1, 3, 4))
    assert not ops._handoff_g16_ready(lk, d_out.clone(), (2, 2, 3, 4))
    assert not ops._handoff_g16_ready(None, d_out, (2, 2, 3, 4))
    d_out.add_(1.0)                                      # another consumer's gradient accumulated in place, or a hook's mul_
    assert d_out.data_ptr() == lk["dx_ptr"]
    assert not ops._handoff_g16_ready(lk, d_out, (2, 2, 3, 4))


def test_a_gradient_hook_that_edits_in_place_keeps_the_address_and_moves_the_version():
    """What the G16 hand-off check relies on, with stock autograd: a Function whose backward returns a view of a fresh buffer, and a
    hook on its input that scales the gradient in place - the next backward receives the same address with a newer version."""
    seen = {}

    class Producer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v):
            return v * 1.0

        @staticmethod
        def backward(ctx, d):
            seen["ptr"], seen["version"] = d.data_ptr(), d._version
            return d

    class Consumer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a):
            return a.sum(-1)

        @staticmethod
        def backward(ctx, g):
            d_x = torch.ones(6, 4)
            seen["dx_ptr"], seen["dx_version"] = d_x.data_ptr(), d_x._version
            return d_x.reshape(2, 3, 4)

    a = Producer.apply(torch.zeros(2, 3, 4, requires_grad=True))
    a.register_hook(lambda gr: gr.mul_(0.5))
    Consumer.apply(a).sum().backward()
    assert seen["ptr"] == seen["dx_ptr"] and seen["version"] != seen["dx_version"]


# --------------------------------------------------------------------------- round 3
def test_importing_ops_or_utils_does_not_fire_the_drop_in_side_effects():
    """the reference's import-time side effects (pit.py:1-11) belong to the drop-in module `pit` only."""
    import subprocess
    code = ("import sys, torch; torch.manual_seed(123); a = torch.rand(1).item();"
            "torch.manual_seed(123); import position_induced_transformer_amd.ops, position_induced_transformer_amd.utils;"
            "assert 'position_induced_transformer_amd.pit' not in sys.modules;"
            "assert torch.rand(1).item() == a;"                    # the global RNG was not reseeded
            "import position_induced_transformer_amd as P; P.pit;"  # lazy attribute: loads (and seeds, as pit.py:3)
            "assert 'position_induced_transformer_amd.pit' in sys.modules;"
            "torch.manual_seed(0); b = torch.rand(1).item(); import importlib;"
            "importlib.reload(sys.modules['position_induced_transformer_amd.pit']); assert torch.rand(1).item() == b")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]


def test_subclass_overrides_of_dist2att_or_convolution_are_detected():
    """pit.py:42-43 calls self.dist2att / self.convolution: a subclass that overrides either must not be bypassed."""
    from position_induced_transformer_amd import pit as P

    class mine(P.posatt_fixed):
        def convolution(self, A, U):
            return 2.0 * super().convolution(A, U)

    class other(P.posatt_cross):
        def dist2att(self, mesh_out, mesh_in, scale, locality):
            return super().dist2att(mesh_out, mesh_in, scale, 1.0)

    for cls in (P.posatt, P.posatt_cross, P.posatt_fixed, P.posatt_cross_fixed, P.posatt_periodic1d,
                P.posatt_cross_periodic1d, P.posatt_periodic2d, P.posatt_cross_periodic2d):
        assert not cls(2, 4, 0.5)._overridden(), cls
    assert mine(2, 4, 0.5)._overridden() and other(2, 4, 0.5)._overridden()
    a, u = torch.rand(2, 5, 7, dtype=torch.float32), torch.rand(3, 7, 4)
    want = torch.einsum("hnj,bjd->bnhd", a.double(), u.double()).reshape(3, 5, 8).float()
    assert torch.equal(P.posatt_fixed(2, 4, 1.0).convolution(a, u), want)          # exact fp64 contraction, rounded once
    assert torch.get_float32_matmul_precision() == "high"                           # (pit.py:2; the helper does not toggle it)


def test_build_is_stale_after_a_build_with_other_flags_and_the_binding_checks_the_abi_version(tmp_path, monkeypatch):
    from position_induced_transformer_amd import _lib, build
    assert not build._stale()
    monkeypatch.setattr(build, "FLAGS", build.FLAGS + ["-DPIT_STAMPS"])
    assert build._stale()                       # a diagnostic build would not be mistaken for this one, nor vice versa
    monkeypatch.undo()
    assert _lib.lib().pit_version() == _lib.ABI_VERSION
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="PIT_ABI_VERSION"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib() is not None


def test_attention_launch_record_reports_its_kinds_and_copies_what_fits():
    """pit_debug_att_counts (PIT_HAS_ATT_COUNTS, an addition to ABI 31): returns the number of PIT_ATT_* slots of the header, copies
    min(n, kinds) of them, accepts out = NULL, and every thread reads a record of its own (all zero here: nothing was launched).
    The non-zero record, its reset and its thread locality are asserted on the GPU (tests/test_gpu_att_edges.py)."""
    import ctypes
    import re
    from position_induced_transformer_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pit_hip.h")).read()
    assert re.search(r"#define PIT_HAS_ATT_COUNTS 1", header)
    assert "pit_debug_att_counts" in _lib.SIGNATURES and "pit_debug_att_counts" in _lib.ADDED_LATER
    slots = {name: int(v) for name, v in re.findall(r"#define PIT_ATT_(\w+)\s+(\d+)\b", header[header.index("#define PIT_HAS_ATT_COUNTS"):])}   # (after the block's marker: the PIT_ATT_UNION math_mode flag stands far above it)
    kinds = slots.pop("KINDS")
    assert sorted(slots.values()) == list(range(kinds))                    # one slot per kind, none twice
    fn = _lib.lib().pit_debug_att_counts
    assert fn(None, 0, 0) == kinds and fn(None, kinds, 1) == kinds
    for n in (0, 3, kinds, kinds + 5):
        buf = (ctypes.c_int * (kinds + 5))(*([-1] * (kinds + 5)))
        assert fn(buf, n, 0) == kinds
        assert list(buf) == [0] * min(n, kinds) + [-1] * (kinds + 5 - min(n, kinds))
    assert ops.att_launch_counts() == [0] * kinds
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.att_launch_counts(reset=True)))
    t.start()
    t.join()
    assert seen == [[0] * kinds]


def test_postponed_job_slices_cover_the_rows_once_and_respect_the_early_bucket():
    """ops._dw_slices: a postponed weight-gradient job cut into row slices for the fused processor's launches - every row
    exactly once, slices 16-row aligned, operand pointers advanced by whole rows; and the number of parts a two-bucket step
    allows (ops._PROCESSOR_HOOK = (callback, complete_by)): only the launches up to the early bucket's reduce."""
    from position_induced_transformer_amd import _lib, ops
    rows, n0, n1, n2 = 14792, 128, 64, 1
    job = _lib.MlpParamsJob(0x10000000, n0, rows, n0, n1, n2, 0x20000000, 0, 0x30000000, n2, 1, 2, 3, 4, 1, 0x40000000, 0)
    for parts in (1, 2, 3, 4):
        sl = ops._dw_slices((job,), parts)
        assert len(sl) <= parts and sum(s.rows for s in sl) == rows
        r0 = 0
        for s in sl:
            assert r0 % 16 == 0 and s.accumulate == 1 and s.out_gelu == 0
            assert s.x == job.x + 4 * r0 * n0 and s.h == job.h + 4 * r0 * n1
            assert s.d_y == job.d_y + 4 * r0 * n2 and s.scratch == job.scratch + 4 * r0 * n1
            assert (s.d_w1, s.d_b1, s.d_w2, s.d_b2) == (1, 2, 3, 4)
            r0 += s.rows
    # the number of launches that may carry a slice: all n blocks, or n - complete_by under a two-bucket step
    n = 4
    for hook, want in ((None, 4), ((lambda i: None, 2), 2), ((lambda i: None, 3), 1), ((lambda i: None, 0), 4)):
        parts = n if hook is None else max(1, n - hook[1])
        assert parts == want


def test_fused_processor_gate_refuses_more_blocks_than_one_weights_launch_forms():
    """pit_block_weights takes at most ops.BLOCK_MAX_LAYERS (16) layers; pit._fused_processor must answer None
    for a deeper processor (the reference accepts any n_blocks) BEFORE anything touches the device."""
    import torch
    from position_induced_transformer_amd import ops, pit as P
    assert ops.BLOCK_MAX_LAYERS == 16
    mesh = torch.rand(256, 2)
    model = P.pit_fixed(2, 1, 1, 64, 2, 17, mesh, 0.02, 0.02)
    calls = []
    orig = ops.block_fusion_supported
    ops.block_fusion_supported = lambda *a: calls.append(a) or True
    try:
        assert model._fused_processor(torch.zeros(2, 256, 64), model.mesh_ltt) is None
    finally:
        ops.block_fusion_supported = orig
    assert not calls


# --------------------------------------------------------------------------- where d(lmda) and an MLP's weight gradients go
# (the keywords a backward node constructs ops._HeadGrad with, as the seven nodes spell them)
HEAD_KINDS = {"fresh": {}, "encoder": {"always_accumulators": True}, "shared": {"shared_workspace": True},
              "kernel": {"shared_workspace": True, "kernel_finishes": True}}


@pytest.mark.parametrize("is_scale", [False, True])
@pytest.mark.parametrize("mode", ["unwanted", "returned", "inplace", "deferred"])
def test_head_gradient_object_over_delivery_modes_and_node_kinds(mode, is_scale, monkeypatch):
    """ops._HeadGrad over {no gradient wanted, returned to autograd, in place now, in place deferred} x {head is lmda, head is the
    scale} x the nodes' keywords: the flags that reach the one finishing launcher (in place = 1 only with a slot, 4 = head is the
    scale), which accumulators the kernel is handed, what finish() returns, what the self-finishing launch gets, and
    _defer_head_begin run by the constructor exactly when deferring."""
    from position_induced_transformer_amd import ops
    slot, param = torch.zeros(2), object()
    shared = torch.zeros(8, dtype=torch.float64)
    launched, flushed, begun = [], [], []
    monkeypatch.setattr(ops, "_grad_slot", lambda p: slot if (p is param and mode in ("inplace", "deferred")) else None)
    monkeypatch.setattr(ops, "DEFER_HEAD_FINISH", mode == "deferred")
    monkeypatch.setattr(ops, "_launch_head_finishes", lambda entries, rider=None: launched.append(list(entries)))
    monkeypatch.setattr(ops, "_flush_head_finishes", lambda task: flushed.extend(ops._PENDING_HEADS.pop(task)))
    monkeypatch.setattr(ops, "_dscale_workspace", lambda device, n_head: shared)
    real_begin = ops._defer_head_begin
    monkeypatch.setattr(ops, "_defer_head_begin", lambda work: (begun.append(work), real_begin(work))[1])
    ops._PENDING_HEADS.clear()
    head, scale = torch.ones(2), torch.ones(2)
    seen = {}

    class Layer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            for kind, kw in HEAD_KINDS.items():
                n0, l0 = len(begun), len(launched)
                hg = ops._HeadGrad(param, mode != "unwanted", 2, torch.device("cpu"), is_scale, **kw)
                begins = len(begun) - n0
                ret = hg.finish(head, scale)
                seen[kind] = (hg, begins, ret, launched[l0:])
            return g * 2

    Layer.apply(torch.ones(3, requires_grad=True)).sum().backward()
    bit = 4 if is_scale else 0
    own = ops._layer_workspace(slot, 2)                              # (cached per gradient slot: the object the constructor took)
    for kind, (hg, begins, ret, launches) in seen.items():
        assert begins == (1 if mode == "deferred" else 0), (kind, "_defer_head_begin")
        assert (hg.slot is slot) == (mode in ("inplace", "deferred")) and hg.defer == (mode == "deferred")
        # accumulators
        if mode == "deferred":
            assert hg.work is own, kind
        elif kind in ("shared", "kernel"):
            assert hg.work is shared, kind
        elif mode == "unwanted" and kind == "fresh":
            assert hg.work is None
        else:
            assert hg.work.dtype == torch.float64 and hg.work.numel() == 2 * 1024 and float(hg.work.abs().sum()) == 0.0, kind
            assert hg.work is not own and hg.work is not shared
        # the gradient tensor and what autograd receives
        if mode == "unwanted":
            assert hg.d_head is None and ret is None and launches == []
            continue
        assert (hg.d_head is slot) if hg.slot is not None else (tuple(hg.d_head.shape) == (2,) and hg.d_head.dtype == torch.float32)
        assert (ret is None) if hg.slot is not None else (ret is hg.d_head), kind
        assert hg.acc == {"returned": 0, "inplace": 1, "deferred": 3}[mode]
        # the finishing launch
        if mode == "deferred" or kind == "kernel":
            assert launches == [], kind
        else:
            (entry,), = launches
            assert entry[0] is hg.work and entry[1] is hg.d_head and entry[2] is head and entry[3] is scale and entry[4] == 2
            assert entry[5] == (1 if mode == "inplace" else 0) | bit, (kind, entry[5])
    if mode == "deferred":                                           # one entry per layer, drained by the pass's one flush
        assert len(flushed) == len(HEAD_KINDS)
        for e in flushed:
            assert e[0] is own and e[1] is slot and e[5] == 1 | bit
    else:
        assert flushed == [] and not ops._PENDING_HEADS


def test_head_gradients_of_one_node_share_one_finishing_launch(monkeypatch):
    """_HeadGrad.finish_all (the fused processor): layers whose gradient is returned or goes in place now are finished by ONE
    launch, in layer order, each with its own flags."""
    from position_induced_transformer_amd import ops
    slot, marked = torch.zeros(2), object()
    launched = []
    monkeypatch.setattr(ops, "_grad_slot", lambda p: slot if p is marked else None)
    monkeypatch.setattr(ops, "DEFER_HEAD_FINISH", False)
    monkeypatch.setattr(ops, "_launch_head_finishes", lambda entries, rider=None: launched.append(list(entries)))
    hgs = [ops._HeadGrad(p, True, 2, torch.device("cpu"), False) for p in (None, marked, None)]
    heads, scales = [torch.ones(2) for _ in hgs], [torch.ones(2) for _ in hgs]
    out = ops._HeadGrad.finish_all(list(zip(hgs, heads, scales)))
    assert len(launched) == 1 and [e[5] for e in launched[0]] == [0, 1, 0]
    assert [e[2] for e in launched[0]] == heads and [e[0] for e in launched[0]] == [g.work for g in hgs]
    assert out[0] is hgs[0].d_head and out[1] is None and out[2] is hgs[2].d_head


@pytest.mark.parametrize("fresh", ["empty", "zeros"])
@pytest.mark.parametrize("case", ["all_slots", "one_slot_missing", "needs_partly_false"])
def test_weight_gradient_tail_over_slots_and_fresh_kinds(case, fresh, monkeypatch):
    """ops._mlp_grad_slots / _params_job / _dw_deliver over {every parameter opted in, one did not, one needs no gradient} x {fresh
    tensors uninitialised (the caller's kernels overwrite them, accumulate 0: _Mlp) or zeroed (the kernels add, accumulate 1: the
    fused nodes)}: the four gradient tensors, the in-place verdict, the job's fields (a job always adds), postponed exactly when in
    place and deferrable, and the four-tuple handed to autograd."""
    from position_induced_transformer_amd import ops
    rows, n0, n1, n2 = 6, 5, 4, 3
    shapes = ((n1, n0), (n1,), (n2, n1), (n2,))
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    slots = {id(p): torch.ones(s) for p, s in zip(params, shapes)}
    if case == "one_slot_missing":
        del slots[id(params[2])]
    needs = (True, True, True, case != "needs_partly_false")
    monkeypatch.setattr(ops, "_grad_slot", lambda p: slots.get(id(p)))
    made = {"zeros": 0, "empty": 0}
    real = {"zeros": torch.zeros, "empty": torch.empty}
    for kind in made:
        monkeypatch.setattr(torch, kind, lambda *a, _k=kind, **k: (made.__setitem__(_k, made[_k] + 1), real[_k](*a, **k))[1])
    grads, inplace = ops._mlp_grad_slots(params, shapes, needs, torch.device("cpu"), fresh=fresh)
    monkeypatch.undo()
    assert inplace == (case == "all_slots")
    if inplace:
        assert all(g is slots[id(p)] for g, p in zip(grads, params)) and made == {"zeros": 0, "empty": 0}
    else:
        assert made == {fresh: 4, ("empty" if fresh == "zeros" else "zeros"): 0}
        assert [tuple(g.shape) for g in grads] == [tuple(s) for s in shapes] and all(g.dtype == torch.float32 for g in grads)
        assert all(all(g is not s for s in slots.values()) for g in grads)
        if fresh == "zeros":
            assert all(float(g.abs().sum()) == 0.0 for g in grads)
    x, h, d_y, scratch = torch.zeros(rows, 8)[:, :n0], torch.zeros(rows, n1), torch.zeros(rows, n2), torch.zeros(rows * (n1 + n2))
    st, keep = ops._params_job(x, h, d_y, scratch, grads, (rows, n0, n1, n2), 1, 0x100)
    assert (st.x, st.ldx, st.rows, st.n0, st.n1, st.n2, st.h, st.out_gelu) == (x.data_ptr(), 8, rows, n0, n1, n2, h.data_ptr(), 1)
    assert (st.d_y, st.ld_dy, st.accumulate, st.scratch, st.math_mode) == (d_y.data_ptr(), n2, 1, scratch.data_ptr(), 0x100)
    assert (st.d_w1, st.d_b1, st.d_w2, st.d_b2) == tuple(g.data_ptr() for g in grads)
    assert all(a is b for a, b in zip(keep, (x, h, d_y, scratch) + tuple(grads)))
    assert ops._params_job(x, h, scratch, scratch, grads, (rows, n0, n1, n2), 1, 0, ld_dy=7)[0].ld_dy == 7
    for deferrable in (True, False):
        for rider in (True, False):
            calls = []
            monkeypatch.setattr(ops, "MLP_PARAMS_RIDER", rider)
            monkeypatch.setattr(ops, "_dw_deferrable", lambda *key: calls.append(("deferrable", key)) or deferrable)
            monkeypatch.setattr(ops, "_dw_defer", lambda st_, keep_, dev: calls.append(("defer", st_, keep_)))
            monkeypatch.setattr(ops, "_dw_run", lambda job: calls.append(("run", job[0], job[1], job[2])))
            monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: "the current stream")
            out = ops._dw_deliver((st, keep), inplace, torch.device("cpu"))
            monkeypatch.undo()
            what = [c for c in calls if c[0] != "deferrable"]
            assert len(what) == 1 and what[0][1] is st and what[0][2] is keep
            assert what[0][0] == ("defer" if (inplace and rider and deferrable) else "run")
            if what[0][0] == "run":
                assert what[0][3] == "the current stream"
            for c in calls:
                if c[0] == "deferrable":
                    assert c[1] == (rows, n0, n1, n2, 1, n2)
            assert isinstance(out, tuple) and len(out) == 4
            assert all(a is None for a in out) if inplace else all(a is b for a, b in zip(out, grads))
