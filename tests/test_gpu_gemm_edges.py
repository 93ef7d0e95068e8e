"""The GEMM core of every MLP and Linear (csrc/pit_mlp.hip, csrc/pit_mlp_slab.hip, csrc/pit_gemm_rd.h) at its tile, slab and stride
edges, one dispatch instance at a time, through the raw C ABI: pit_linear_fwd / _bwd, pit_mlp_fwd / _bwd_data / _bwd_params / _bwd.

Every GPU case

* resets the library's launch record (pit_debug_gemm_counts, include/pit_hip.h), runs ONE entry and asserts the exact record -
  kind -> number of launches, and for the fused kernels the template arguments the record holds.  The expectation is the `expect`
  argument of the case (entry -> record), never re-derived from the dispatch rule;
* hands every tensor as a view inside a larger allocation pre-filled with the NaN bit pattern FILL: 64 guard rows before and after
  the view, `pad` guard columns between rows wherever the entry takes a leading dimension.  After the call every word outside an
  output's view still holds FILL (`Band.untouched`), and inputs keep NaN in their padding columns, so a kernel that lets padding
  into a K tail or a row tail turns its result NaN;
* compares every output with an fp64 evaluation of the same formula on the CPU (erf-gelu MLP, pit.py:21-26; for the backward from
  the fp32 Z1, H, Z2 the entry was given) PER 32 x 32 BLOCK (`block_err`): rel-L2 of each block with the tensor's RMS as the floor of
  the denominator; the last partial row and column blocks are blocks of their own.  Bounds are the project's, per block: forward
  2e-6, data and weight gradients 1e-5 (fp32 mode), 2e-2 / 5e-2 (bf16 math mode, tests/test_gpu_bf16.py).

`test_block_comparison_sees_what_a_global_norm_hides` (CPU) plants a wrong 1 x 64 strip and a dropped 64-row K chunk in correct
results and shows which comparison flags what.

Case ids and the kinds they assert (names = PIT_GEMM_* of include/pit_hip.h, lower case):

* ``lin-*``      pit_linear_fwd + pit_linear_bwd below the LDS thresholds: rd_tn1 (BIAS, STORE, ATOMIC), ``lin-tn2-*`` rd_tn2
* ``lds-*``      the LDS-tiled kernels: lds_32 / lds_64 / lds_128 (fp32 mode), bfl_32 / bfl_64 / bfl_128 (bf16 mode), lds_agz,
                 mul_gelu_grad; the ids carry tile height and epilogue
* ``rr-*``       rr (pit_linear_bwd) and rr_pair (pit_mlp_bwd_params above 2^28)
* ``pair-*`` / ``triple-*``  rd_pair, rd_triple_tn1, rd_triple_tn2
* ``f16-*``      mlp_fwd16 / mlp_bwd16 with last_fwd16 = N1 * 100 + KS, last_bwd16 = N1 * 100 + TPW
* ``slab-*``     mlp_fwd64 / mlp_bwd64 (+ _thin) with last_fwd64 = KS, last_bwd64 = T
* ``thin-*``     thin_fwd, thin_fwd_stream, thin_dz1, thin_dw

Instances the default dispatch cannot reach (listed, not forced):

* ``gemm_lds_kernel<128, false, false, EPI_ATOMIC, false>`` and ``gemm_bfl_kernel<128, false, false, EPI_ATOMIC, false>`` (fp32 storage):
  try_launch_gemm_lds picks the row-reducing kind only when a_ic and b_ic hold and both operands are 16-byte aligned, which is
  word for word what gemm_rr_ok asks - gemm_rr_kernel takes every such reduction in both math modes unless PIT_NO_GEMM_RR (or
  PIT_NO_GEMM_RR_BF16) is set;
* ``gemm_rr_kernel<1, 2, 32>`` (64 x 128 tiles) and every other PIT_RR_CFG tile: an environment switch for experiments;
* ``gemm_lds_kernel<..., BF = true>``: PIT_BF16_LEGACY in PIT_EXPERIMENTS builds only;
* ``gemm_bfl_kernel<..., IO16 = true>`` (kind bfl_io16): bf16 STORAGE, which has its own modules and is out of scope here;
* the second work limit of launch_gemm_bwd_tail, dX alone above 2^27: dW1's work rows * n1 * (n0 + 1) exceeds dX's rows * n0 * n1, so
  dX > 2^27 implies a total above 2^28 and the first limit has already decided - the condition is dead code, and only 2^28 is
  bracketed (``triple-tn2-below-2p28`` / ``triple-above-2p28``).

Mutation check (scratch builds, one change each, the cases of the touched kernel re-run): dropping the row-tail mask of the 32-row
gemm_lds epilogue turned 9 ``lds-*`` cases red (guard rows written); launching 8 gx (gy / 8) workgroups under the XCD remap 16
``lds-*`` cases (every remapped case with gy % 8 != 0: NaN left in the last row tiles); streaming thin_fwd at K > 4 tpr
``thin-fwd-no-stream-65536x260x2``; reading ldx as n0 in mlp_fwd16 the four ``f16-*`` forwards with a padded x.  Two mutants are
equivalent: gemm_rr_kernel without the min(K, .) on its last chunk, and without the early exit of the padding workgroups - the
tile's loads go through buffer descriptors sized to K rows (a row >= K is out of range and reads 0), and a padding workgroup has
an empty k range and adds 0.0 to a tile that exists.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import golden_io as gio

FILL = 0x7FC0BEEF                       # a quiet NaN with a recognisable payload
GUARD = 64                              # guard rows before and after every view
TOL_FWD, TOL_GRAD = 2e-6, 1e-5          # fp32 mode, per block
TOL_FWD_BF, TOL_GRAD_BF = 2e-2, 5e-2    # bf16 math mode (tests/test_gpu_bf16.py: TOL_OUT, TOL_GRAD)
FP32, BF16 = 0, 1                       # PIT_MATH_*

KINDS = ("rd_tn1", "rd_tn2", "rd_pair", "rd_triple_tn1", "rd_triple_tn2", "lds_32", "lds_64", "lds_128", "lds_agz", "bfl_32", "bfl_64",
         "bfl_128", "bfl_io16", "rr", "rr_pair", "mul_gelu_grad", "thin_dz1", "thin_fwd", "thin_fwd_stream", "thin_dw", "mlp_fwd16",
         "mlp_bwd16", "mlp_fwd64", "mlp_fwd64_thin", "mlp_bwd64", "mlp_bwd64_thin", "last_fwd16", "last_bwd16", "last_fwd64",
         "last_bwd64")                  # PIT_GEMM_* in order


# --------------------------------------------------------------------------- block-wise comparison (CPU)
def block_err(got, ref, bs=32):
    """max over the bs x bs blocks of a 2-D tensor of ||got - ref||_block / max(||ref||_block, rms(ref) sqrt(block size)); the last
    partial row / column blocks count as blocks of their own.  inf if `got` holds a NaN or an inf.  The sums run in fp64 on the
    device `got` lives on (the reference itself always comes from the CPU)."""
    got = torch.as_tensor(got)
    got, ref = got.double(), torch.as_tensor(ref).to(got.device).double()
    if got.dim() == 1:
        got, ref = got[None, :], ref[None, :]
    assert got.shape == ref.shape and got.dim() == 2
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    r, c = ref.shape
    rb, cb = (r + bs - 1) // bs, (c + bs - 1) // bs

    def sums(t):                                          # per-block sums of a (r, c) tensor
        p = torch.zeros(rb * bs, cb * bs, dtype=torch.float64, device=t.device)
        p[:r, :c] = t
        return p.view(rb, bs, cb, bs).sum(dim=(1, 3))
    num, den = sums((got - ref) ** 2), sums(ref ** 2)
    rows_in = torch.clamp(r - bs * torch.arange(rb, device=got.device), max=bs).double()
    cols_in = torch.clamp(c - bs * torch.arange(cb, device=got.device), max=bs).double()
    floor = torch.clamp(rows_in[:, None] * cols_in[None, :] * float((ref ** 2).mean()), min=1e-300)
    return float(torch.sqrt(num / torch.maximum(den, floor)).max())


def rel_l2(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).norm() / ref.norm())


def test_block_comparison_sees_what_a_global_norm_hides():
    """Two defects of the size a mis-masked tile leaves, planted in correct fp64 results.

    1. A forward of 16 384 rows x 64 columns whose LAST ROW (one 1 x 64 strip) lost its K tail (the last 4 of 36 terms).
    2. A weight gradient (256 x 256, a reduction over 9 999 rows) where ONE 64 x 64 tile lost one 64-row K chunk.

    Whole-tensor rel-L2: 3.9e-3 and 2.0e-2; worst block: 8.8e-2 and 8.1e-2.  Both are above the fp32 bounds, so at 2e-6 / 1e-5 the global norm sees them as well - what
    it cannot do is tell a tile from a tensor: at the bounds of the bf16 math mode (2e-2 forward, 5e-2 gradients), which are the
    project's bounds for half of the cases of this module, both pass the global norm and neither passes the block comparison; and
    the global figure shrinks with the tensor (the strip: 1 / sqrt(rows)) while the block figure does not."""
    x, w = torch.from_numpy(gio.synth((16384, 36), 11)).double(), torch.from_numpy(gio.synth((64, 36), 12)).double()
    ref = x @ w.T
    bad = ref.clone()
    bad[-1] = x[-1, :32] @ w[:, :32].T
    assert rel_l2(bad, ref) < TOL_FWD_BF < block_err(bad, ref)
    assert block_err(ref.float(), ref) < TOL_FWD                     # (and a correctly rounded result passes the fp32 bound)
    small = slice(16384 - 512, 16384)                                # the same strip in 512 rows: the global norm moves, the block does not
    assert rel_l2(bad[small], ref[small]) > 5 * rel_l2(bad, ref)
    assert abs(block_err(bad[small], ref[small]) / block_err(bad, ref) - 1) < 0.2

    dz, xx = torch.from_numpy(gio.synth((9999, 256), 13)).double(), torch.from_numpy(gio.synth((9999, 256), 14)).double()
    ref = dz.T @ xx
    bad = ref.clone()
    bad[64:128, 128:192] -= dz[9920:9984, 64:128].T @ xx[9920:9984, 128:192]
    assert rel_l2(bad, ref) < TOL_GRAD_BF < block_err(bad, ref)
    assert block_err(ref.float(), ref) < TOL_GRAD


# --------------------------------------------------------------------------- guard bands
class Band:
    """A (rows, n) fp32 view with row pitch ld = n + pad, `off` floats off the 16-byte grid, inside one allocation filled with FILL:
    GUARD rows before and after it.  `data` (a CPU tensor) makes it an input: the view holds the data, its padding stays NaN."""

    def __init__(self, rows, n, pad=0, off=0, data=None):
        self.rows, self.n, self.ld = rows, n, n + pad
        self.start = GUARD * self.ld + off
        self.buf = torch.full(((rows + 2 * GUARD) * self.ld + off + 4,), FILL, dtype=torch.int32, device="cuda")
        self.t = self.buf.view(torch.float32).as_strided((rows, n), (self.ld, 1), self.start)
        if data is not None:
            self.t.copy_(data.reshape(rows, n).float())
        assert self.t.data_ptr() % 16 == 4 * (off % 4)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        """Every word outside the view is still FILL."""
        c = self.buf.clone()
        c.as_strided((self.rows, self.n), (self.ld, 1), self.start).fill_(FILL)
        return bool((c == FILL).all())

    def unwritten(self):
        """... and the view too (an output the entry must leave alone)."""
        return bool((self.buf == FILL).all())

    def cpu(self):
        return self.t.cpu()


def counts(reset=True):
    from position_induced_transformer_amd import ops
    c = ops.gemm_launch_counts(reset=reset)
    assert len(c) == len(KINDS)
    return {k: v for k, v in zip(KINDS, c) if v}


def _call(entry, *args):
    from position_induced_transformer_amd import _lib
    rc = getattr(_lib.lib(), entry)(*args)
    _lib.check(rc, entry)


def _stream():
    from position_induced_transformer_amd import _lib
    return _lib.stream_ptr()


def _bounds(mode):
    return (TOL_FWD, TOL_GRAD) if mode == FP32 else (TOL_FWD_BF, TOL_GRAD_BF)


def check(name, band, ref, tol, report):
    """One output: guard band intact, every block within tol.  Figures are printed before they are asserted."""
    err = block_err(band.t, ref)
    print(f"  {name}: block err {err:.3e} (bound {tol:.0e})")
    report.append((name, err, tol, band.untouched()))


def settle(report):
    torch.cuda.synchronize()
    for name, err, tol, clean in report:
        assert clean, f"{name}: wrote outside its view"
        assert err <= tol, f"{name}: block err {err:.3e} > {tol:.0e}"


# --------------------------------------------------------------------------- fp64 references (computed once per shape, never modified)
def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _t(shape, seed, scale=1.0):
    return torch.from_numpy(gio.synth(shape, seed) * np.float32(scale))


@functools.lru_cache(maxsize=2)
def linear_case(rows, n_in, n_out):
    """fp32 inputs of one Linear and its fp64 forward / backward (d_w includes the accumulate = 1 seed w0)."""
    s = 7 * rows + 131 * n_in + 1009 * n_out
    x, w, dy, w0 = _t((rows, n_in), s), _t((n_out, n_in), s + 1, math.sqrt(2.0 / n_in)), _t((rows, n_out), s + 2), _t((n_out, n_in), s + 3)
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    return dict(x=x, w=w, dy=dy, w0=w0, y=x64 @ w64.T, dx=dy64 @ w64, dw=dy64.T @ x64)


@functools.lru_cache(maxsize=2)
def mlp_case(rows, n0, n1, n2, gelu):
    """fp32 inputs of one kaiming_mlp (pit.py:21-26), its fp64 forward, and the fp64 backward from the fp32-rounded Z1, H, Z2 the
    backward entries are given.  dw* / db* include the accumulate = 1 seeds."""
    s = 3 * rows + 17 * n0 + 257 * n1 + 4099 * n2 + gelu
    x, dy = _t((rows, n0), s), _t((rows, n2), s + 1)
    w1, w2 = _t((n1, n0), s + 2, math.sqrt(2.0 / n0)), _t((n2, n1), s + 3, math.sqrt(2.0 / n1))
    b1 = torch.from_numpy(gio.synth((n1,), s + 4, -1.0 / math.sqrt(n0), 1.0 / math.sqrt(n0)))
    b2 = torch.from_numpy(gio.synth((n2,), s + 5, -1.0 / math.sqrt(n1), 1.0 / math.sqrt(n1)))
    seeds = dict(dw1=_t((n1, n0), s + 6), db1=_t((n1,), s + 7), dw2=_t((n2, n1), s + 8), db2=_t((n2,), s + 9))
    z1 = x.double() @ w1.double().T + b1.double()
    h = gelu64(z1)
    z2 = h @ w2.double().T + b2.double()
    y = gelu64(z2) if gelu else z2
    z1f, hf, z2f = z1.float(), h.float(), z2.float()
    dz2 = dy.double() * gelu_grad64(z2f.double()) if gelu else dy.double()
    dz1 = (dz2 @ w2.double()) * gelu_grad64(z1f.double())
    return dict(x=x, dy=dy, w1=w1, b1=b1, w2=w2, b2=b2, seeds=seeds, z1=z1, h=h, z2=z2, y=y, z1f=z1f, hf=hf, z2f=z2f, dz2=dz2, dz1=dz1,
                dx=dz1 @ w1.double(), dw2=dz2.T @ hf.double(), db2=dz2.sum(0), dw1=dz1.T @ x.double(), db1=dz1.sum(0))


# --------------------------------------------------------------------------- runners
gpu = pytest.mark.gpu


def _pad(n, pad):
    """'odd': the smallest pad >= 1 that makes the row pitch odd (so never a multiple of 4)."""
    return (1 if n % 2 == 0 else 2) if pad == "odd" else pad


def run_linear(c):
    """pit_linear_fwd (c['fwd'] = expected record) and / or pit_linear_bwd (c['bwd']) of one case; returns the non-atomic outputs."""
    rows, k, n = c["shape"]
    mode, pad, off, acc = c.get("mode", FP32), c.get("pad", 0), c.get("off", 0), c.get("acc", 0)
    tf, tg = _bounds(mode)
    ref, rep, out = linear_case(rows, k, n), [], {}
    x, w = Band(rows, k, _pad(k, pad), off, ref["x"]), Band(n, k, 0, off, ref["w"])
    if "fwd" in c["run"]:
        zb, y = Band(1, n, data=torch.zeros(n)), Band(rows, n, _pad(n, pad))
        counts()
        _call("pit_linear_fwd", x.ptr, x.ld, rows, k, n, w.ptr, zb.ptr, y.ptr, y.ld, mode, _stream())
        got = counts()
        print(f"  fwd record {got}")
        assert got == c["expect"]["fwd"]
        check("y", y, ref["y"], tf, rep)
        out["y"] = y.t
    if "bwd" in c["run"]:
        dy = Band(rows, n, _pad(n, pad), off, ref["dy"])
        dx = Band(rows, k, _pad(k, pad)) if c.get("dx", True) else None
        dw = Band(n, k, data=ref["w0"] if acc else None) if c.get("dw", True) else None
        counts()
        _call("pit_linear_bwd", x.ptr, x.ld, rows, k, n, w.ptr, dy.ptr, dy.ld, dx.ptr if dx else None, dx.ld if dx else k,
              dw.ptr if dw else None, acc, mode, _stream())
        got = counts()
        print(f"  bwd record {got}")
        assert got == c["expect"]["bwd"]
        if dx:
            check("d_x", dx, ref["dx"], tg, rep)
            out["dx"] = dx.t
        if dw:
            check("d_w", dw, ref["dw"] + (ref["w0"].double() if acc else 0.0), tg, rep)
    settle(rep)
    return out


def run_mlp(c):
    """The entries of one MLP case that carry an expected record: c['fwd'], c['bwd_data'], c['bwd_params'], c['bwd']."""
    rows, n0, n1, n2 = c["shape"]
    mode, pad, acc, gelu = c.get("mode", FP32), c.get("pad", 0), c.get("acc", 0), c.get("gelu", 0)
    off = c.get("off", {})                                  # floats off the 16-byte grid, per tensor
    tf, tg = _bounds(mode)
    ref, rep = mlp_case(rows, n0, n1, n2, gelu), []
    x = Band(rows, n0, _pad(n0, c.get("pad_x", pad)), off.get("x", 0), ref["x"])
    w1, w2 = Band(n1, n0, 0, off.get("w1", 0), ref["w1"]), Band(n2, n1, 0, off.get("w2", 0), ref["w2"])
    if "fwd" in c["run"]:
        b1, b2 = Band(1, n1, data=ref["b1"]), Band(1, n2, data=ref["b2"])
        z1, h, z2, y = Band(rows, n1), Band(rows, n1), Band(rows, n2), Band(rows, n2, _pad(n2, pad))
        counts()
        _call("pit_mlp_fwd", x.ptr, x.ld, rows, n0, n1, n2, w1.ptr, b1.ptr, w2.ptr, b2.ptr, gelu, z1.ptr, h.ptr, z2.ptr, y.ptr, y.ld,
              mode, _stream())
        got = counts()
        print(f"  fwd record {got}")
        assert got == c["expect"]["fwd"]
        check("z1", z1, ref["z1"], tf, rep)
        check("h", h, ref["h"], tf, rep)
        check("y", y, ref["y"], tf, rep)
        if gelu:
            check("z2", z2, ref["z2"], tf, rep)
        else:
            assert z2.unwritten(), "z2 written without a trailing gelu"
    for entry in ("bwd_data", "bwd_params", "bwd"):
        if entry not in c["run"]:
            continue
        z1, h = Band(rows, n1, data=ref["z1f"]), Band(rows, n1, data=ref["hf"])
        z2 = Band(rows, n2, data=ref["z2f"]) if gelu else None
        dy = Band(rows, n2, _pad(n2, c.get("pad_dy", 0 if gelu else pad)), off.get("dy", 0), ref["dy"])    # (ld_dy == n2 with a gelu)
        dx = Band(rows, n0, _pad(n0, pad)) if c.get("dx", True) and entry != "bwd_params" else None
        scratch = Band(rows, n1 + n2)                       # dZ1 (rows, n1) | dZ2 (rows, n2), contiguous
        flat = scratch.t.view(-1)
        dz1, dz2 = flat[:rows * n1].view(rows, n1), flat[rows * n1:].view(rows, n2)
        grads = None
        if entry != "bwd_data":
            seeds = ref["seeds"]
            grads = dict(dw1=Band(n1, n0, data=seeds["dw1"] if acc else None), db1=Band(1, n1, data=seeds["db1"] if acc else None),
                         dw2=Band(n2, n1, data=seeds["dw2"] if acc else None), db2=Band(1, n2, data=seeds["db2"] if acc else None))
        if entry == "bwd_params":
            dz1.copy_(ref["dz1"].float())
            if gelu:
                dz2.copy_(ref["dz2"].float())
        counts()
        if entry == "bwd_data":
            _call("pit_mlp_bwd_data", rows, n0, n1, n2, w1.ptr, w2.ptr, z1.ptr, z2.ptr if z2 else None, gelu, dy.ptr, dy.ld,
                  dx.ptr if dx else None, dx.ld if dx else n0, scratch.ptr, mode, _stream())
        elif entry == "bwd_params":
            _call("pit_mlp_bwd_params", x.ptr, x.ld, rows, n0, n1, n2, h.ptr, gelu, dy.ptr, dy.ld, grads["dw1"].ptr, grads["db1"].ptr,
                  grads["dw2"].ptr, grads["db2"].ptr, acc, scratch.ptr, mode, _stream())
        else:
            _call("pit_mlp_bwd", x.ptr, x.ld, rows, n0, n1, n2, w1.ptr, w2.ptr, z1.ptr, h.ptr, z2.ptr if z2 else None, gelu, dy.ptr, dy.ld,
                  dx.ptr if dx else None, dx.ld if dx else n0, grads["dw1"].ptr, grads["db1"].ptr, grads["dw2"].ptr, grads["db2"].ptr,
                  acc, scratch.ptr, mode, _stream())
        got = counts()
        print(f"  {entry} record {got}")
        assert got == c["expect"][entry]
        assert scratch.untouched(), "scratch: wrote outside dZ1 | dZ2"
        if entry != "bwd_params":
            e1 = block_err(dz1, ref["dz1"])
            print(f"  dz1: block err {e1:.3e}")
            rep.append((entry + " dz1", e1, tg, True))
            if gelu:
                e2 = block_err(dz2, ref["dz2"])
                print(f"  dz2: block err {e2:.3e}")
                rep.append((entry + " dz2", e2, tg, True))
            else:
                assert bool((dz2.view(torch.int32) == FILL).all()), "dZ2 written without a trailing gelu"
            if dx:
                check(entry + " d_x", dx, ref["dx"], tg, rep)
        if grads:
            for name, band in grads.items():
                want = ref[name] + (ref["seeds"][name].double() if acc else 0.0)
                check(entry + " " + name, band, want.reshape(band.rows, band.n), tg, rep)
    settle(rep)


# --------------------------------------------------------------------------- cases
def _case(kind, cid, shape, kw):
    """`expect`: entry -> the launch record it must leave (kind -> launches; last_* = template arguments).  Its keys are the entries run."""
    c = dict(id=cid, kind=kind, shape=shape, **kw)
    c.setdefault("run", tuple(c.get("expect", ())))
    return c


def _lin(cid, rows, k, n, **kw):
    return _case("lin", cid, (rows, k, n), kw)


def _mlp(cid, rows, n0, n1, n2, **kw):
    return _case("mlp", cid, (rows, n0, n1, n2), kw)


def _slab_rows(ks, tail):
    """The smallest row count above the fused 16-row kernels' work limit (rows * 64 * (n0 + 64) > 2^27) with rows % 64 == tail."""
    rows = (1 << 27) // (64 * (16 * ks + 64)) + 1
    return rows + (tail - rows) % 64


CASES = [
    # ---- register-direct (gemm_rd_kernel) through pit_linear_*: BIAS (fwd), STORE (d_x), ATOMIC without a ones column (d_w).
    # K of the three GEMMs = n_in, n_out, rows: 1 .. 130 covers 2, 4 and 8 waves and k tails off the 8-grid
    _lin("lin-m1-k1-n1", 1, 1, 1, pad="odd", 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m31-k7-n31", 31, 7, 31, pad="odd", 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m32-k8-n33", 32, 8, 33, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m33-k9-n65", 33, 9, 65, pad="odd", 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m33-k31-n1", 33, 31, 1, pad=4, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m31-k33-n65", 31, 33, 65, pad="odd", acc=1, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m32-k64-n31", 32, 64, 31, pad="odd", 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m33-k130-n33", 33, 130, 33, pad="odd", acc=1, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m130-k64-n64", 130, 64, 64, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-m130-k64-n64-bf16", 130, 64, 64, mode=BF16, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-tn2-bias-8197x24x130", 8197, 24, 130, pad="odd", 
         expect=dict(fwd={'rd_tn2': 1}, bwd={'rd_tn1': 2})),
    _lin("lin-tn2-store-8197x130x24", 8197, 130, 24, 
         expect=dict(fwd={'rd_tn1': 1}, bwd={'rd_tn1': 1, 'rd_tn2': 1})),
    _lin("lin-tn2-atomic-33x513x1825", 33, 513, 1825, 
         expect=dict(bwd={'rd_tn2': 1}), dx=False),
    # ---- LDS-tiled kernels through pit_linear_*: BIAS = forward, STORE = d_x alone.  M one past a tile multiple
    _lin("lds-32-bias-4097x260x130", 4097, 260, 130, pad=4, 
         expect=dict(fwd={'lds_32': 1})),      # remap, gy = 129
    _lin("lds-32-bias-4097x260x130-bf16", 4097, 260, 130, pad=4, mode=BF16, 
         expect=dict(fwd={'bfl_32': 1})),
    _lin("lds-64-bias-16769x260x65", 16769, 260, 65, 
         expect=dict(fwd={'lds_64': 1})),      # remap, gy = 263 (gy % 8 = 7)
    _lin("lds-64-bias-16769x260x65-bf16", 16769, 260, 65, mode=BF16, 
         expect=dict(fwd={'bfl_64': 1})),
    _lin("lds-128-bias-13185x64x320", 13185, 64, 320, pad=8, 
         expect=dict(fwd={'lds_128': 1})),      # remap, gy = 104 (gy % 8 = 0)
    _lin("lds-128-bias-13185x64x320-bf16", 13185, 64, 320, pad=8, mode=BF16, 
         expect=dict(fwd={'bfl_128': 1})),
    _lin("lds-64-bias-k36-28737x36x130", 28737, 36, 130, 
         expect=dict(fwd={'lds_64': 1})),
    _lin("lds-64-bias-k36-28737x36x130-bf16", 28737, 36, 130, mode=BF16, 
         expect=dict(fwd={'bfl_64': 1})),
    _lin("lds-64-bias-k4-258113x4x130", 258113, 4, 130, 
         expect=dict(fwd={'lds_64': 1})),
    _lin("lds-32-bias-noremap-1985x1060x64", 1985, 1060, 64, 
         expect=dict(fwd={'lds_32': 1})),      # gx = 1, gy = 63
    _lin("lds-32-bias-noremap-1985x1060x64-bf16", 1985, 1060, 64, mode=BF16, 
         expect=dict(fwd={'bfl_32': 1})),
    _lin("lds-n48-11001x260x48", 11001, 260, 48, 
         expect=dict(fwd={'lds_32': 1})),
    _lin("lds-n47-refused-11001x260x47", 11001, 260, 47, 
         expect=dict(fwd={'rd_tn1': 1})),
    _lin("lds-work-2p27-8192x256x64", 8192, 256, 64, 
         expect=dict(fwd={'lds_32': 1})),
    _lin("lds-work-below-2p27-8191x256x64", 8191, 256, 64, 
         expect=dict(fwd={'rd_tn1': 1})),
    _lin("lds-32-store-4097x132x260", 4097, 132, 260, pad=4, 
         expect=dict(bwd={'lds_32': 1}), dw=False),
    _lin("lds-32-store-4097x132x260-bf16", 4097, 132, 260, pad=4, mode=BF16, 
         expect=dict(bwd={'bfl_32': 1}), dw=False),
    _lin("lds-64-store-16769x68x260", 16769, 68, 260, 
         expect=dict(bwd={'lds_64': 1}), dw=False),
    _lin("lds-64-store-16769x68x260-bf16", 16769, 68, 260, mode=BF16, 
         expect=dict(bwd={'bfl_64': 1}), dw=False),
    _lin("lds-128-store-13185x320x64", 13185, 320, 64, 
         expect=dict(bwd={'lds_128': 1}), dw=False),
    _lin("lds-128-store-13185x320x64-bf16", 13185, 320, 64, mode=BF16, 
         expect=dict(bwd={'bfl_128': 1}), dw=False),
    _lin("lds-refused-ldx-odd-4097x260x130", 4097, 260, 130, pad="odd", 
         expect=dict(fwd={'rd_tn1': 1})),
    # ---- LDS-tiled kernels through the MLP entries: BIAS_GELU (forward) and MUL_GELU_GRAD (dZ1: AGZ at K = n2 <= 128 in fp32 mode,
    # the separate pass above that and in bf16 mode)
    _mlp("lds-32-mlp-agz-8001x132x132x128", 8001, 132, 132, 128, gelu=1, 
         expect=dict(fwd={'lds_32': 2}, bwd_data={'lds_32': 2, 'lds_agz': 1})),
    _mlp("lds-32-mlp-agz-8001x132x132x128-bf16", 8001, 132, 132, 128, gelu=1, mode=BF16, 
         expect=dict(fwd={'bfl_32': 2}, bwd_data={'bfl_32': 2, 'mul_gelu_grad': 1})),
    _mlp("lds-32-mlp-pass-8001x132x132x132", 8001, 132, 132, 132, gelu=1, 
         expect=dict(bwd_data={'lds_32': 2, 'mul_gelu_grad': 1})),
    _mlp("lds-64-mlp-agz-16769x120x68x120", 16769, 120, 68, 120, gelu=1, 
         expect=dict(fwd={'lds_64': 2}, bwd_data={'lds_64': 2, 'lds_agz': 1})),
    _mlp("lds-64-mlp-agz-16769x120x68x120-bf16", 16769, 120, 68, 120, gelu=1, mode=BF16, 
         expect=dict(fwd={'bfl_64': 2}, bwd_data={'bfl_64': 2, 'mul_gelu_grad': 1})),
    _mlp("lds-128-mlp-agz-13185x64x320x64", 13185, 64, 320, 64, gelu=1, 
         expect=dict(fwd={'lds_32': 1, 'lds_128': 1}, bwd_data={'lds_32': 1, 'lds_128': 1, 'lds_agz': 1})),
    _mlp("lds-128-mlp-agz-13185x64x320x64-bf16", 13185, 64, 320, 64, gelu=1, mode=BF16, 
         expect=dict(fwd={'bfl_32': 1, 'bfl_128': 1}, bwd_data={'bfl_32': 1, 'bfl_128': 1, 'mul_gelu_grad': 1})),
    _mlp("lds-128-mlp-pass-13185x64x320x132", 13185, 64, 320, 132, gelu=1, 
         expect=dict(bwd_data={'lds_32': 1, 'lds_128': 1, 'mul_gelu_grad': 1})),
    _mlp("lds-128-mlp-nogelu-13185x64x320x64", 13185, 64, 320, 64, gelu=0, pad_dy=4, 
         expect=dict(bwd_data={'lds_32': 1, 'lds_128': 1})),
    # ---- gemm_rr_kernel: single through pit_linear_bwd (d_w alone; M = n_out, n_real = n_in, K = rows)
    _lin("rr-m32-n48-r87423", 87423, 48, 32, 
         expect=dict(bwd={'rr': 1}), dx=False),      # rows % 64 = 63, one tile
    _lin("rr-m32-n48-r87423-bf16", 87423, 48, 32, mode=BF16, 
         expect=dict(bwd={'rr': 1}), dx=False),
    _lin("rr-m96-n68-r20608-acc", 20608, 68, 96, acc=1, pad=4, 
         expect=dict(bwd={'rr': 1}), dx=False),      # rows % 64 = 0
    _lin("rr-m100-n192-r7041-percu1", 7041, 192, 100, 
         expect=dict(bwd={'rr': 1}), dx=False),      # rows % 64 = 1, 6 tiles x 42 slabs: P % 8 = 4
    _lin("rr-m100-n192-r7041-percu1-bf16", 7041, 192, 100, mode=BF16, 
         expect=dict(bwd={'rr': 1}), dx=False),
    _lin("rr-m100-n192-r43583-percu2", 43583, 192, 100, acc=1, 
         expect=dict(bwd={'rr': 1}), dx=False),
    _lin("rr-refused-m98-n192-r7169", 7169, 192, 98, 
         expect=dict(bwd={'rd_tn1': 1}), dx=False),      # M % 4 != 0 at work >= 2^27
    # ... paired (both reductions of one MLP, ones-column bias sums) through pit_mlp_bwd_params above 2^28, rd_pair just below
    _mlp("rr-pair-27595x68x96x32", 27595, 68, 96, 32, 
         expect=dict(bwd_params={'rr_pair': 1})),
    _mlp("rr-pair-27595x68x96x32-bf16", 27595, 68, 96, 32, mode=BF16, 
         expect=dict(bwd_params={'rr_pair': 1})),
    _mlp("pair-below-2p28-27594x68x96x32", 27594, 68, 96, 32, 
         expect=dict(bwd_params={'rd_pair': 1})),
    _mlp("rr-pair-gelu-acc-27649x68x96x32", 27649, 68, 96, 32, gelu=1, acc=1, pad_x=4, 
         expect=dict(bwd_params={'rr_pair': 1})),
    _mlp("rr-pair-refused-ldx-odd-27649x68x96x32", 27649, 68, 96, 32, pad_x="odd", 
         expect=dict(bwd_params={'rd_tn1': 2})),
    _mlp("rr-pair-refused-m98-27649x68x98x32", 27649, 68, 98, 32, 
         expect=dict(bwd_params={'rd_tn1': 2})),      # n1 % 4 != 0 above 2^28
    # ---- pair and triple (register-direct, one launch) at widths the fused kernels refuse
    _mlp("pair-255x20x48x8", 255, 20, 48, 8, 
         expect=dict(bwd_params={'rd_pair': 1}, bwd={'rd_tn1': 1, 'rd_pair': 1}), dx=False),
    _mlp("triple-255x20x48x8-gelu", 255, 20, 48, 8, gelu=1, 
         expect=dict(bwd={'rd_tn1': 1, 'rd_triple_tn1': 1})),
    _mlp("triple-300x33x130x7", 300, 33, 130, 7, pad_x="odd", pad_dy="odd", acc=1, 
         expect=dict(bwd={'rd_tn1': 1, 'rd_triple_tn1': 1})),
    _mlp("pair-300x33x130x7-gelu", 300, 33, 130, 7, gelu=1, 
         expect=dict(bwd={'rd_tn1': 1, 'rd_pair': 1}), dx=False),
    _mlp("triple-tn2-8197x130x48x8", 8197, 130, 48, 8, 
         expect=dict(bwd={'rd_tn1': 1, 'rd_triple_tn2': 1})),
    _mlp("triple-tn2-below-2p28-20776x130x48x8", 20776, 130, 48, 8, 
         expect=dict(bwd={'rd_tn2': 1, 'rd_triple_tn2': 1})),
    _mlp("triple-above-2p28-20777x130x48x8", 20777, 130, 48, 8, 
         expect=dict(bwd={'rd_tn2': 2, 'rd_pair': 1})),
    # ---- fused 16-row kernels
    _mlp("f16-n32-256x1x32x1", 256, 1, 32, 1, pad="odd", 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3204}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 3201}, bwd={'rd_pair': 1, 'mlp_bwd16': 1, 'last_bwd16': 3201})),
    _mlp("f16-n32-257x15x32x4-gelu", 257, 15, 32, 4, gelu=1, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3204}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 3201})),
    _mlp("f16-n32-271x17x32x16", 271, 17, 32, 16, pad="odd", 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3204}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 3201})),
    _mlp("f16-n32-271x80x32x32-gelu", 271, 80, 32, 32, gelu=1, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3208}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 3203}, bwd={'rd_pair': 1, 'mlp_bwd16': 1, 'last_bwd16': 3203})),
    _mlp("f16-n32-257x128x32x16", 257, 128, 32, 16, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3208}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 3204})),
    _mlp("f16-n32-256x48x32x16", 256, 48, 32, 16, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3204}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 3202})),
    _mlp("f16-n32-256x200x32x4-bwd-refused", 256, 200, 32, 4, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3216})),
    _mlp("f16-n64-256x100x64x16", 256, 100, 64, 16, pad="odd", 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 6408}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 6402})),
    _mlp("f16-n128-257x100x128x16", 257, 100, 128, 16, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 12808}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 12801})),
    _mlp("f16-n128-257x192x128x4-gelu", 257, 192, 128, 4, gelu=1, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 12812}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 12802})),
    _mlp("f16-n32-256x129x32x16-bwd-refused", 256, 129, 32, 16, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 3212}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n32-256x16x32x5-refused", 256, 16, 32, 5, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n32-256x16x32x24-refused", 256, 16, 32, 24, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n32-256x16x32x48-refused", 256, 16, 32, 48, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n64-256x16x64x64-gelu", 256, 16, 64, 64, gelu=1, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 6404}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 6401})),
    _mlp("f16-n64-271x192x64x4", 271, 192, 64, 4, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 6412}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 6403})),
    _mlp("f16-n64-257x256x64x1-gelu", 257, 256, 64, 1, gelu=1, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 6416}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 6404})),
    _mlp("f16-n64-256x257x64x16-refused", 256, 257, 64, 16, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n64-257x256x64x80-refused", 257, 256, 64, 80, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n128-255x16x128x128-refused", 255, 16, 128, 128, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n128-256x17x128x128-gelu", 256, 17, 128, 128, gelu=1, pad="odd", 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 12804}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 12801})),
    _mlp("f16-n128-271x256x128x16", 271, 256, 128, 16, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 12816}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 12802})),
    _mlp("f16-n128-256x16x128x144-refused", 256, 16, 128, 144, 
         expect=dict(fwd={'rd_tn1': 2}, bwd_data={'rd_tn1': 2})),
    _mlp("f16-n128-work-2p27-4096x252x128x4", 4096, 252, 128, 4, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 12816}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 12802})),
    _mlp("f16-n128-work-above-2p27-4097x252x128x4", 4097, 252, 128, 4, 
         expect=dict(fwd={'rd_tn1': 1, 'thin_fwd': 1}, bwd_data={'rd_tn2': 1, 'thin_dz1': 1})),
    _mlp("f16-n64-ld-dy-257x48x64x16", 257, 48, 64, 16, pad_dy=3, 
         expect=dict(bwd_data={'mlp_bwd16': 1, 'last_bwd16': 6401}, bwd={'rd_pair': 1, 'mlp_bwd16': 1, 'last_bwd16': 6401})),
    _mlp("f16-n64-bf16-257x48x64x16", 257, 48, 64, 16, mode=BF16, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 6404}, bwd_data={'mlp_bwd16': 1, 'last_bwd16': 6401})),
    _mlp("f16-refused-w2-misaligned-257x48x64x16", 257, 48, 64, 16, off={"w2": 1}, 
         expect=dict(fwd={'rd_tn1': 2})),
    _mlp("f16-x-w1-misaligned-257x48x64x16", 257, 48, 64, 16, off={"x": 1, "w1": 1}, 
         expect=dict(fwd={'mlp_fwd16': 1, 'last_fwd16': 6404})),
]
# ---- slab kernels (fp32 mode, hid 64): every KS = n0 / 16 (and with it every T = ceil(n0 / 64) of the backward) at the smallest
# row counts above the 16-row kernels' limit that leave row tails of 1 and of 63
for _ks in range(1, 17):
    for _tail in (1, 63):
        _r = _slab_rows(_ks, _tail)
        CASES.append(_mlp(f"slab-ks{_ks}-{_r}x{16 * _ks}x64x64", _r, 16 * _ks, 64, 64, gelu=(_ks + _tail // 63) % 2, pad=4 * (_ks % 3),
                          expect=dict(fwd={"mlp_fwd64": 1, "last_fwd64": _ks},
                                      bwd_data={"mlp_bwd64": 1, "last_bwd64": (_ks + 3) // 4})))
CASES += [
    _mlp("slab-bwd-26241x16x64x64", 26241, 16, 64, 64, gelu=1, 
         expect=dict(bwd={'rd_pair': 1, 'mlp_bwd64': 1, 'last_bwd64': 1})),
    _mlp("slab-preferred-walk-65537x16x64x64", 65537, 16, 64, 64, gelu=1, 
         expect=dict(fwd={'mlp_fwd64': 1, 'last_fwd64': 1}, bwd_data={'mlp_bwd64': 1, 'last_bwd64': 1})),      # 1025 slabs > 2 x CUs
    _mlp("slab-preferred-bf16-65599x32x64x64", 65599, 32, 64, 64, mode=BF16, 
         expect=dict(fwd={'mlp_fwd64': 1, 'last_fwd64': 2}, bwd_data={'mlp_bwd64': 1, 'last_bwd64': 1})),
    _mlp("slab-below-preferred-65535x16x64x64", 65535, 16, 64, 64, mode=BF16, 
         expect=dict(fwd={'rd_tn2': 1, 'bfl_64': 1})),
    _mlp("slab-thin-262144x16x64x1", 262144, 16, 64, 1, 
         expect=dict(fwd={'mlp_fwd64_thin': 1, 'last_fwd64': 1}, bwd_data={'mlp_bwd64_thin': 1, 'last_bwd64': 1})),
    _mlp("slab-thin-262144x16x64x4-gelu", 262144, 16, 64, 4, gelu=1, 
         expect=dict(fwd={'mlp_fwd64_thin': 1, 'last_fwd64': 1}, bwd_data={'mlp_bwd64_thin': 1, 'last_bwd64': 1})),
    _mlp("slab-thin-refused-262143x16x64x4", 262143, 16, 64, 4, 
         expect=dict(fwd={'lds_64': 1, 'thin_fwd_stream': 1}, bwd_data={'rd_tn1': 1, 'thin_dz1': 1})),
    _mlp("slab-refused-ldx-odd-26241x16x64x64", 26241, 16, 64, 64, pad_x="odd", 
         expect=dict(fwd={'rd_tn2': 2})),
    _mlp("slab-refused-x-misaligned-26241x16x64x64", 26241, 16, 64, 64, off={"x": 1}, 
         expect=dict(fwd={'rd_tn2': 2})),
    _mlp("slab-refused-w1-misaligned-26241x16x64x64", 26241, 16, 64, 64, off={"w1": 1}, 
         expect=dict(fwd={'rd_tn2': 2})),
    _mlp("slab-refused-dy-misaligned-26241x16x64x64", 26241, 16, 64, 64, off={"dy": 1}, 
         expect=dict(bwd_data={'rd_tn1': 1, 'rd_tn2': 1})),
    _mlp("slab-refused-n0-24-23873x24x64x64", 23873, 24, 64, 64, 
         expect=dict(fwd={'rd_tn2': 2}, bwd_data={'rd_tn1': 1, 'rd_tn2': 1})),      # above the 16-row limit for n0 = 24
    # ---- thin kernels
    _lin("thin-fwd-stream-131072x4x1", 131072, 4, 1, pad=4, 
         expect=dict(fwd={'thin_fwd_stream': 1})),      # rows * K = 2^19, tpr 4
    _lin("thin-fwd-refused-131071x4x1", 131071, 4, 1, 
         expect=dict(fwd={'rd_tn1': 1})),      # 2^19 - K
    _lin("thin-fwd-tpr4-32768x16x2", 32768, 16, 2, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-tpr8-26215x20x3", 26215, 20, 3, pad=4, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-tpr16-8192x64x4", 8192, 64, 4, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-refused-8191x64x4", 8191, 64, 4, 
         expect=dict(fwd={'rd_tn1': 1})),
    _lin("thin-fwd-tpr32-4096x128x1", 4096, 128, 1, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-tpr64-3972x132x2", 3972, 132, 2, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-loop-2017x260x3", 2017, 260, 3, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-stream-65536x16x4", 65536, 16, 4, 
         expect=dict(fwd={'thin_fwd_stream': 1})),
    _lin("thin-fwd-plain-65535x16x4", 65535, 16, 4, 
         expect=dict(fwd={'thin_fwd': 1})),
    _lin("thin-fwd-no-stream-65536x260x2", 65536, 260, 2, 
         expect=dict(fwd={'thin_fwd': 1})),      # K > tpr * 4: the looping form
    _lin("thin-fwd-refused-k-odd-32768x18x2", 32768, 18, 2, 
         expect=dict(fwd={'rd_tn1': 1})),
    _mlp("thin-mlp-gelu-10923x20x48x3", 10923, 20, 48, 3, gelu=1, 
         expect=dict(fwd={'rd_tn1': 1, 'thin_fwd': 1}, bwd_data={'rd_tn1': 1, 'thin_dz1': 1})),      # thin_fwd with gelu; thin_dz1 keeps dZ2
    _mlp("thin-dz1-10923x20x48x4", 10923, 20, 48, 4, 
         expect=dict(bwd_data={'rd_tn1': 1, 'thin_dz1': 1})),      # rows * n1 >= 2^19
    _mlp("thin-dz1-refused-10922x20x48x4", 10922, 20, 48, 4, 
         expect=dict(bwd_data={'rd_tn1': 2})),
    _mlp("thin-dz1-refused-n1-50-10923x20x50x4", 10923, 20, 50, 4, 
         expect=dict(bwd_data={'rd_tn1': 2})),
    _mlp("thin-dw-8192x256x128x4", 8192, 256, 128, 4, 
         expect=dict(bwd_params={'rr': 1, 'thin_dw': 1})),
    _mlp("thin-dw-refused-8191x256x128x4", 8191, 256, 128, 4, 
         expect=dict(bwd_params={'rd_tn1': 1, 'rr': 1})),
    _mlp("thin-dw-one-row-slab-8449x256x128x1-gelu", 8449, 256, 128, 1, gelu=1, acc=1, 
         expect=dict(bwd_params={'rr': 1, 'thin_dw': 1})),
    _mlp("thin-dw-8192x256x128x2", 8192, 256, 128, 2, 
         expect=dict(bwd_params={'rr': 1, 'thin_dw': 1})),
    _mlp("thin-dw-8192x256x128x3", 8192, 256, 128, 3, 
         expect=dict(bwd_params={'rr': 1, 'thin_dw': 1})),
]


def test_every_kind_has_a_case():
    """(CPU) case ids are unique, and every PIT_GEMM_* kind but bfl_io16 (bf16 storage: out of scope) is asserted by some case."""
    assert len({c["id"] for c in CASES}) == len(CASES) and all(c["expect"] for c in CASES)
    records = [rec for c in CASES for rec in c["expect"].values()]
    seen = {k for rec in records for k in rec}
    assert seen == set(KINDS) - {"bfl_io16"}
    with open(__file__.replace("tests/test_gpu_gemm_edges.py", "include/pit_hip.h")) as f:
        header = f.read()
    import re
    names = re.findall(r"#define PIT_GEMM_(\w+)\s+(\d+)", header)
    assert [n.lower() for n, _ in names[:-1]] == list(KINDS)
    assert names[-1] == ("KINDS", str(len(KINDS)))
    last = lambda slot: {rec[slot] for rec in records if slot in rec}
    assert last("last_fwd16") == {n1 * 100 + ks for n1 in (32, 64, 128) for ks in (4, 8, 12, 16)}         # every <N1, KS>
    assert last("last_bwd16") == {n1 * 100 + tpw for n1, most in ((32, 4), (64, 4), (128, 2)) for tpw in range(1, most + 1)}
    assert last("last_fwd64") == set(range(1, 17)) and last("last_bwd64") == {1, 2, 3, 4}


@gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_case(case):
    (run_linear if case["kind"] == "lin" else run_mlp)(case)


@gpu
def test_misaligned_base_pointers_take_the_scalar_loads_and_change_nothing():
    """x, w and d_y one float off the 16-byte grid (a_vec = b_vec = 0 in gemm_rd_kernel: 4-byte fragment loads): the same kernels,
    and the outputs that are not summed with atomics keep their bits."""
    base = _lin("aligned", 33, 64, 65, expect=dict(fwd={"rd_tn1": 1}, bwd={"rd_tn1": 2}))
    a = run_linear(base)
    b = run_linear(dict(base, id="misaligned", off=1))
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["dx"], b["dx"])


@gpu
def test_trailing_gelu_with_padded_d_y_is_refused_before_any_launch():
    """include/pit_hip.h: ld_dy == n2 when out_gelu.  Every fused kernel steps aside for ld_dy != n2 and the GEMM path answers
    PIT_ERR_SIZE: nothing is launched, nothing written (pit_mlp_bwd_data; fused-eligible and slab-eligible shapes)."""
    from position_induced_transformer_amd import _lib
    for rows, n0, n1, n2 in ((257, 48, 64, 16), (26241, 16, 64, 64), (300, 20, 48, 8)):
        ref = mlp_case(rows, n0, n1, n2, 1)
        w1, w2 = Band(n1, n0, data=ref["w1"]), Band(n2, n1, data=ref["w2"])
        z1, z2, dy = Band(rows, n1, data=ref["z1f"]), Band(rows, n2, data=ref["z2f"]), Band(rows, n2, 4, data=ref["dy"])
        dx, scratch = Band(rows, n0), Band(rows, n1 + n2)
        counts()
        rc = _lib.lib().pit_mlp_bwd_data(rows, n0, n1, n2, w1.ptr, w2.ptr, z1.ptr, z2.ptr, 1, dy.ptr, dy.ld, dx.ptr, dx.ld, scratch.ptr,
                                         FP32, _stream())
        torch.cuda.synchronize()
        assert rc == -2 and counts() == {}                       # PIT_ERR_SIZE
        assert dx.unwritten() and scratch.unwritten()
