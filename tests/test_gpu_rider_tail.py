"""GPU: the weight-gradient riders of pit_block_bwd (csrc/pit_block.hip) after the rider-tail change - the thin dW2 | db2 of a
postponed job with at most four output rows as a vector-ALU row reduction (thin_rider, csrc/pit_gemm_rd.h), and the gemm_rr_tile
tiles of the block's own MLP dealt to the XCD that holds their sample's rows - against an fp64 CPU evaluation.

pit_block_bwd is called through the C ABI as bench.roofline_block_probe does, on a 16 x 16 latent grid (L = 256), D = 64; every
gradient buffer is pre-filled with seeded non-zero values (the riders accumulate).  Bound: the rel-L2 5e-7 that
tests/test_gpu_grad_delivery.py (TOL_WEIGHT) applies to the same weight gradients.  One gradient of the parent commit misses it at
these shapes: db2 of an n2 = 1 layer is ONE number, pre-fill + the sum of the rows' N(0, 1) d_y, and where that sum nearly cancels
its relative error is a few units in the last place of the partial sums - the parent measured 7.61e-7 (259 rows, ld_dy 1, where
the value is 1.07; every other figure of the parent is at most 2.6e-7), so that gradient is allowed
twice the parent's figure (TOL_DB2_SCALAR); this commit measured 5.78e-7 there.  Every figure is printed before it is asserted.
"""
import ctypes
import functools

import pytest
import torch

import golden_io as gio
from test_gpu_fused_envelope import _model, lattice

pytestmark = pytest.mark.gpu

D, SHAPE, L = 64, (16, 16), 256
TOL_WEIGHT = 5e-7               # tests/test_gpu_grad_delivery.py: TOL_WEIGHT
TOL_DB2_SCALAR = 2 * 7.61e-7    # db2 with n2 = 1: twice the parent commit's measured error (module docstring)
THIN_ROWS = (1, 17, 255, 259, 3698, 4600)


@functools.lru_cache(maxsize=None)
def _weights(heads):
    """(E, Q, inv) of one layer on the regular 16 x 16 grid with a fresh model's lmda."""
    from position_induced_transformer_amd import ops
    mesh = lattice(SHAPE, 90, jitter=0.0)
    model = _model("euclid", 2, 1, 1, D, heads, 1, mesh, 0.02, 91)
    plan = model.conv[0]._plan(model.mesh_ltt, model.mesh_ltt, True)
    E, Q, inv, _rowstat, _scale, _heads = ops.block_weights(plan, [model.conv[0].lmda], heads, need_q=True)
    torch.cuda.synchronize()
    return E[0].contiguous(), Q[0].contiguous(), inv[0].contiguous()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


class _Job:
    """One pit_mlp_params_job on seeded operands: the ctypes struct, the pre-filled gradient buffers, and their fp64 values."""

    def __init__(self, g, rows, n0, n1, n2, out_gelu, ld_dy):
        from position_induced_transformer_amd import _lib
        x, h, dz1 = _randn(g, rows, n0), _randn(g, rows, n1), _randn(g, rows, n1)
        dy = _randn(g, rows, ld_dy)
        dz2 = _randn(g, rows, n2) if out_gelu else dy[:, :n2]           # (out_gelu: dZ2 sits behind dZ1 in the scratch)
        pre = [_randn(g, n1, n0), _randn(g, n1), _randn(g, n2, n1), _randn(g, n2)]
        self.expect = [pre[0].double() + dz1.double().t() @ x.double(), pre[1].double() + dz1.double().sum(0),
                       pre[2].double() + dz2.double().t() @ h.double(), pre[3].double() + dz2.double().sum(0)]
        scratch = torch.cat([dz1.reshape(-1), dz2.reshape(-1)]) if out_gelu else dz1.reshape(-1)
        self.keep = [t.contiguous().cuda() for t in (x, h, dy, scratch)]
        self.grads = [t.cuda() for t in pre]
        xd, hd, dyd, sd = self.keep
        self.job = _lib.MlpParamsJob(xd.data_ptr(), n0, rows, n0, n1, n2, hd.data_ptr(), out_gelu, dyd.data_ptr(), ld_dy,
                                     *[t.data_ptr() for t in self.grads], 1, sd.data_ptr(), 0)

    def ptr(self):
        return ctypes.cast(ctypes.pointer(self.job), ctypes.c_void_p)

    def errors(self):
        return [gio.rel_l2(e.numpy(), t.double().cpu().numpy()) for e, t in zip(self.expect, self.grads)]

    def bounds(self):
        return [TOL_WEIGHT, TOL_WEIGHT, TOL_WEIGHT, TOL_DB2_SCALAR if self.expect[3].numel() == 1 else TOL_WEIGHT]

    def within_bounds(self):
        return all(e <= b for e, b in zip(self.errors(), self.bounds()))


@functools.lru_cache(maxsize=None)
def _chain_operands(heads, batch):
    """Seeded operands of the launch's chain (d(values) of a block + the previous MLP's data path), on the device; never modified."""
    g = torch.Generator().manual_seed(92 + 7 * batch + heads)
    W, rows = (1 + heads) * D, batch * L
    t = {"dxc": _randn(g, rows, W), "xc": _randn(g, rows, W), "z1": _randn(g, rows, D), "z2": _randn(g, rows, D),
         "w1": _randn(g, D, W) / W ** 0.5, "w2": _randn(g, D, D) / D ** 0.5}
    return {k: v.cuda() for k, v in t.items()}


def _block_bwd(heads, batch, rider=None, rider2=None):
    """One pit_block_bwd with d(scale) and the previous MLP in its chain, as in the step: (d_xprev, dZ1 | dZ2 of the previous MLP)."""
    from position_induced_transformer_amd import _lib
    W, rows = (1 + heads) * D, batch * L
    E, Q, inv = _weights(heads)
    c = _chain_operands(heads, batch)
    dxp = torch.full((rows, W), -7.25, device="cuda")
    scr = torch.full((rows * 2 * D,), -7.25, device="cuda")
    ws = torch.zeros(heads * 1024, device="cuda", dtype=torch.float64)
    rc = _lib.lib().pit_block_bwd(E.data_ptr(), inv.data_ptr(), Q.data_ptr(), L, heads, D, batch, c["dxc"].data_ptr(), c["xc"].data_ptr(),
                                  ws.data_ptr(), c["w1"].data_ptr(), c["w2"].data_ptr(), c["z1"].data_ptr(), c["z2"].data_ptr(), 1, W,
                                  dxp.data_ptr(), W, scr.data_ptr(), None, 0, rider.ptr() if rider else None,
                                  rider2.ptr() if rider2 else None, 0, _lib.stream_ptr())
    _lib.check(rc, "pit_block_bwd")
    torch.cuda.synchronize()
    return dxp, scr


def _last_riders():
    """(register-direct, tile, thin workgroups, XCD-local map used, d(scale) slabs first) of the most recent pit_block_bwd."""
    from position_induced_transformer_amd import _lib
    out = (ctypes.c_int * 5)()
    assert _lib.lib().pit_block_bwd_last_riders(out, 5) == 5
    return tuple(out)


def _rider_tail_on():
    import os
    return os.environ.get("PIT_RIDER_TAIL", "1")[:1] != "0"


@pytest.mark.parametrize("ld_extra", [0, 2])
@pytest.mark.parametrize("n2", [1, 3])
def test_thin_rider2_matches_fp64(n2, ld_extra):
    """The decoder slice's shape (128 -> 64 -> n2, no trailing gelu) as rider2 of a batch-1 launch: rows 1 and 17 (less than one
    wave instruction per wave), 255 (one workgroup, every load of both stages in range), 259 (two workgroups, a second stage that
    is partly out of range), 3 698 (the flagship slice: 16 workgroups of 231 or 232 rows) and 4 600 (288 rows per workgroup: a
    third stage, the only case in which the two-deep loop goes round twice); d_y rows n2 and n2 + 2 floats apart (the latter never 16-byte aligned).  dW2 | db2 come from the thin body,
    dW1 | db1 of the same job from its tiles.  Parent commit at these shapes (same seeds, rel-L2 against fp64, worst over the 24
    cases): dW1 1.87e-7, db1 2.32e-7, dW2 2.09e-7, db2 2.56e-7 at n2 = 3 and 7.61e-7 at n2 = 1 (module docstring); this commit:
    1.87e-7, 2.24e-7, 1.30e-7, 1.75e-7 and 5.78e-7."""
    g = torch.Generator().manual_seed(93 + 10 * n2 + ld_extra)
    for rows in THIN_ROWS:
        job = _Job(g, rows, 128, D, n2, 0, n2 + ld_extra)
        _block_bwd(2, 1, rider2=job)
        errs = job.errors()
        kinds = _last_riders()
        print(f"thin n2={n2} ld_dy={n2 + ld_extra} rows={rows}: dW1 {errs[0]:.3e} db1 {errs[1]:.3e} dW2 {errs[2]:.3e} db2 {errs[3]:.3e} "
              f"(bounds {job.bounds()}); workgroups rd/tile/thin/local/ds-first {kinds}")
        if _rider_tail_on():
            assert kinds[2] == max(1, min(16, rows // 128)) and kinds[0] == 0, (rows, kinds)
        assert job.within_bounds(), (rows, errs)


@pytest.mark.parametrize("batch", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("heads", [1, 2])
def test_own_dw_tiles_match_fp64(heads, batch):
    """The block's own MLP ((1 + H) 64 -> 64 -> 64, trailing gelu) as `rider`: batch 8 deals the tiles to their sample's XCD, the
    other batches keep the id / tiles map (fewer samples than XCDs).  A dropped or doubled tile changes dW1 | dW2 by a slab's share.
    Parent commit (same seeds, worst over the cases): dW1 1.67e-7, db1 1.89e-7, dW2 1.67e-7, db2 2.07e-7; this commit: 1.65e-7,
    1.94e-7, 1.66e-7, 1.96e-7."""
    g = torch.Generator().manual_seed(94 + 7 * batch + heads)
    W = (1 + heads) * D
    job = _Job(g, batch * L, W, D, D, 1, D)
    _block_bwd(heads, batch, rider=job)
    errs = job.errors()
    kinds = _last_riders()
    print(f"own H={heads} batch={batch}: dW1 {errs[0]:.3e} db1 {errs[1]:.3e} dW2 {errs[2]:.3e} db2 {errs[3]:.3e} (bound {TOL_WEIGHT:.1e}); "
          f"workgroups rd/tile/thin/local/ds-first {kinds}")
    if _rider_tail_on():
        assert kinds[3] == (1 if batch == 8 else 0), kinds
    assert kinds[1] == (1 + heads + 1) * max(1, batch * L // 128), kinds
    assert job.within_bounds(), errs


def test_chain_outputs_do_not_depend_on_the_riders():
    """Batch 8, H = 2, both riders (the step's launch): d_xprev, dZ1 and dZ2 equal bit for bit those of a launch without riders."""
    g = torch.Generator().manual_seed(95)
    own, thin = _Job(g, 8 * L, 3 * D, D, D, 1, D), _Job(g, 3698, 128, D, 1, 0, 1)
    plain = _block_bwd(2, 8)
    with_riders = _block_bwd(2, 8, rider=own, rider2=thin)
    kinds = _last_riders()
    print("riders rd/tile/thin/local/ds-first", kinds, "own", own.errors(), "thin", thin.errors())
    if _rider_tail_on():
        assert kinds == (0, 64 + 58, 16, 1, 1), kinds         # (138 riders, 10 of them beyond the 128 d(scale) slabs)
    for a, b in zip(plain, with_riders):
        assert torch.equal(a, b)
    assert own.within_bounds() and thin.within_bounds()
