"""GPU: the stacked 8-row form of pit_block_fwd (two heads in the M dimension of one MFMA, csrc/pit_block.hip) against the 16-row
form it replaces at n_head = 2, n_pts = 256, batch <= 8.

Both forms add the same products in the same order (the k-steps of a wave, waves 0..7, then * 1/rowsum) and MFMA output rows do
not mix, so the comparison is EXACT: torch.equal on everything the launch writes.  Setup: a 16 x 16 latent grid (L = 256), D = 64,
E / inv from pit_block_weights with a model's initial lmda, seeded N(0, 1) operands.  The forms are chosen with
pit_block_fwd_set_form and told apart with pit_block_fwd_last_rows (include/pit_hip.h); every test restores form 0."""
import functools

import pytest
import torch

from test_gpu_fused_envelope import _check_processor_grads, _model, _processor_parts, _processor_reference, _rel, lattice

pytestmark = pytest.mark.gpu

D = 64
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _weights(shape, heads):
    """(E, inv) of one layer on the regular `shape` grid with a fresh model's lmda (computed once per mesh and head count)."""
    from position_induced_transformer_amd import ops
    mesh = lattice(shape, 80, jitter=0.0)
    model = _model("euclid", len(shape), 1, 1, D, heads, 1, mesh, 0.02, 81)
    plan = model.conv[0]._plan(model.mesh_ltt, model.mesh_ltt, True)
    E, _q, inv, _rowstat, _scale, _heads = ops.block_weights(plan, [model.conv[0].lmda], heads, need_q=False)
    torch.cuda.synchronize()
    return E[0].contiguous(), inv[0].contiguous()


@functools.lru_cache(maxsize=None)
def _operands(L, heads, batch):
    """Seeded N(0, 1) block input (batch * L, D) and MLP parameters, on the device; never modified."""
    g = torch.Generator().manual_seed(82 + 7 * batch + heads)
    W = (1 + heads) * D
    x = torch.randn(batch * L, D, generator=g)
    w1, b1, w2, b2 = torch.randn(D, W, generator=g), torch.randn(D, generator=g), torch.randn(D, D, generator=g), torch.randn(D, generator=g)
    return tuple(t.cuda() for t in (x, w1 / W ** 0.5, b1, w2 / D ** 0.5, b2))


def _block_fwd(shape, heads, batch, out_gelu=1, ldy=D):
    """One pit_block_fwd through the C ABI on fresh, sentinel-filled buffers: {name: tensor} of everything it may write."""
    from position_induced_transformer_amd import _lib
    L, W = shape[0] * shape[1], (1 + heads) * D
    E, inv = _weights(shape, heads)
    x, w1, b1, w2, b2 = _operands(L, heads, batch)
    rows = batch * L
    xcat = torch.full((rows, W), SENTINEL, device="cuda")
    xcat[:, :D] = x
    out = {"xcat": xcat, "y": torch.full((rows, ldy), SENTINEL, device="cuda")}
    for name in ("z1", "h", "z2"):
        out[name] = torch.full((rows, D), SENTINEL, device="cuda")
    rc = _lib.lib().pit_block_fwd(E.data_ptr(), inv.data_ptr(), L, heads, D, batch, xcat.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                  w2.data_ptr(), b2.data_ptr(), out_gelu, out["z1"].data_ptr(), out["h"].data_ptr(),
                                  out["z2"].data_ptr(), out["y"].data_ptr(), ldy, 0, _lib.stream_ptr())
    _lib.check(rc, "pit_block_fwd")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ldy", [64, 192])
@pytest.mark.parametrize("out_gelu", [0, 1])
@pytest.mark.parametrize("batch", [1, 3, 8])
def test_stacked_form_writes_the_bits_of_the_16_row_form(batch, out_gelu, ldy):
    """H = 2, L = 256: batch 1 and 3 leave padded workgroup ids that must return at once, batch 8 is the exact 256-workgroup fit;
    ldy = 192 writes y into the first 64 columns of the next block's concat buffer, as the step does.  xcat, z1, h, z2 (when
    written) and y are equal bit for bit; columns 64.. of the wide y buffer and an unwanted z2 keep their sentinel."""
    from position_induced_transformer_amd import _lib
    L_ = _lib.lib()
    try:
        L_.pit_block_fwd_set_form(16)
        ref = _block_fwd((16, 16), 2, batch, out_gelu, ldy)
        assert L_.pit_block_fwd_last_rows() == 16
        assert L_.pit_block_fwd_set_form(8) == 16
        got = _block_fwd((16, 16), 2, batch, out_gelu, ldy)
        assert L_.pit_block_fwd_last_rows() == 8
    finally:
        L_.pit_block_fwd_set_form(0)
    for name in ("xcat", "z1", "h", "z2", "y"):
        assert torch.isfinite(ref[name]).all(), name
        assert torch.equal(got[name], ref[name]), f"{name}: {int((got[name] != ref[name]).sum())} elements differ"
    for o in (ref, got):
        assert not bool((o["xcat"] == SENTINEL).any()) and not bool((o["z1"] == SENTINEL).any()) and not bool((o["h"] == SENTINEL).any())
        assert not bool((o["y"][:, :D] == SENTINEL).any())
        assert bool((o["y"][:, D:] == SENTINEL).all()), "y columns beyond dim were written"
        if out_gelu:
            assert not bool((o["z2"] == SENTINEL).any())
        else:
            assert bool((o["z2"] == SENTINEL).all()), "z2 written without out_gelu"


def test_dispatch_takes_the_stacked_form_only_inside_its_gate():
    """Form 0: 8 rows for (H 2, L 256, b 8); 16 for b 9 (the 8-row grid would exceed the CUs), H 1, L 512, and after set_form(16)."""
    from position_induced_transformer_amd import _lib
    L_ = _lib.lib()
    prev = L_.pit_block_fwd_set_form(0)
    try:
        assert prev in (0, 8, 16) and L_.pit_block_fwd_set_form(3) < 0 and L_.pit_block_fwd_set_form(0) == 0
        for shape, heads, batch, rows in (((16, 16), 2, 8, 8), ((16, 16), 2, 9, 16), ((16, 16), 1, 8, 16), ((16, 32), 2, 1, 16)):
            _block_fwd(shape, heads, batch)
            assert L_.pit_block_fwd_last_rows() == rows, (shape, heads, batch)
        L_.pit_block_fwd_set_form(16)
        _block_fwd((16, 16), 2, 8)
        assert L_.pit_block_fwd_last_rows() == 16
    finally:
        L_.pit_block_fwd_set_form(0)


def test_backward_consumes_what_the_stacked_forward_saved():
    """ops.processor_apply, 2 blocks, H 2, L 256, batch 3, forward + backward on the default (stacked) form against the oracle's
    processor at the bounds of test_gpu_fused_envelope: output 1e-5 (fp32 oracle), d(input) and weight gradients 2e-5, d(lmda)
    2e-4 (fp64 oracle) - block by block of the largest, and as one vector."""
    from position_induced_transformer_amd import _lib, ops
    mesh = lattice((16, 16), 83)
    model = _model("euclid", 2, 1, 1, D, 2, 2, mesh, 0.02, 84)
    g = torch.Generator().manual_seed(85)
    x = torch.randn(3, 256, D, generator=g)
    d_out = torch.randn(x.shape, generator=g)
    lmdas, mlps = _processor_parts(model)
    ref, _out64, ref_grads = _processor_reference("euclid", mesh, x, d_out, lmdas, mlps)
    plan = model.conv[0]._plan(model.mesh_ltt, model.mesh_ltt, True)
    xg = x.cuda().requires_grad_(True)
    _lib.lib().pit_block_fwd_set_form(0)
    with ops.head_scale_route("host"):
        out = ops.processor_apply(xg, plan, 2, lmdas, mlps)
        assert _lib.lib().pit_block_fwd_last_rows() == 8
        out.backward(d_out.cuda())
    torch.cuda.synchronize()
    print(f"output {_rel(out, ref):.3e}")
    assert _rel(out, ref) <= 1e-5
    grads = [t.detach().cpu() for t in [xg.grad] + [p.grad for p in lmdas] + [t.grad for m in mlps for t in m]]
    _check_processor_grads(grads, ref_grads, 2)
    lm, lm_ref = torch.cat([t.reshape(-1) for t in grads[1:3]]), torch.cat([t.reshape(-1) for t in ref_grads[1:3]])
    print(f"d(lmda) as one vector: {_rel(lm, lm_ref):.3e}")
    assert _rel(lm, lm_ref) <= 2e-4
