"""The folded decoder's kernels (csrc/pit_fold.hip: fold_fwd_kernel, fold_bwd_kernel, fold_reduce_kernel, thin_tail_fwd / _bwd /
_finish_kernel) and the weight tiles they read (pit_fold_weights: decoder_weights_kernel of csrc/pit_edge.hip in its tall-slab mode)
one dispatch instance at a time, through the raw C ABI: pit_fold_weights, pit_fold_att_fwd / _bwd, pit_thin_tail_fwd / _bwd.  The
instance of these entries is a pure function of the arguments - heads, math mode, plan.rows, union_slots(max_union), the io flags,
(n1, n2) - so there is no launch record to assert; every fold case asserts the (rows, max_union, n_slabs) MeshPlan.fold_plan()
returned against its literals instead, so a change to plan building cannot silently move a case to another instance.

Every case

* hands every tensor an entry reads or writes as a `Buf` view (tests/test_gpu_att_edges.py) inside an allocation pre-filled with a
  NaN pattern: guard rows before and after, ld > width, a gap between samples; outputs carry the pattern in their payload too.  After
  the call every word outside an output's view still holds the pattern and every payload element is finite.  pw / qw / pw16 / qw16
  are NaN before pit_fold_weights, `tiles` is NaN before the backward, d_vw is NaN before the tiles form (fold_reduce_kernel must
  write every (sample, key) row, a key no slab holds included) and a known tensor before the atomic form (the entry adds; the rows
  of keys that no slab holds carry -0.0 words, which an add of +0.0 would turn into +0.0: they must keep their bits);
* compares with an fp64 evaluation on the CPU from the operator's definition (as `reference` of test_gpu_att_edges.py: fp32 squared
  distances, orc.row_order_stats, the fp32 lerp threshold, an injected head scale c; no score within 4 ulp of its threshold):
  P_h, Q_h = P_h (m - mbar_h), z = sum_h P_h VW_h, d(VW_h) = P_h^T dZ, d(c_h) = -sum (Q_h VW_h) . dZ, VW head-interleaved;
* fp32 math mode: per block of 4 rows x 64 columns forward 2e-6, d(values) 1e-5, d(c) 1e-4 (TOL of test_gpu_att_edges.py); weight
  tiles 2e-6, exactly 0 in slots >= nkeys[s] and rows >= n_out; pw16 / qw16 equal pw.bfloat16() / qw.bfloat16() bit for bit;
* bf16 math mode: the fp64 reference is evaluated on the operands as the kernel rounds them - the pw16 / qw16 tiles the weights
  kernel produced (verified just before), vw.bfloat16(), dz.bfloat16() - so what is left is fp32 accumulation and the output's storage
  rounding: fp32-stored outputs keep the fp32 bounds, a bf16-stored z gets 2^-8 per block (half an ulp, relative);
* d(scale): the entry adds -tot into PIT_DSCALE_SLOTS fp64 slots per head (guarded like the rest); their fp64 sum is d(c).

Fold instances covered, as (heads, mode, um, rows, n_slabs), each forward + backward in BOTH forms (tiles + fold_reduce_kernel,
fp32 atomics), d(scale) alone and d(values) alone:
  fp32: (1, 32, 256, 9) (2, 32, 256, 1) (1, 48, 256, 3) (2, 48, 128, 8) (1, 64, 64, 5) (2, 64, 256, 6) (2, 48, 64, 7: bf16-stored z
  and dz with fp32 math) (2, 64, 128, 8: a 2-d grid pair); fold_reduce_kernel widths 64, 128, 256 and, on the one-slab mesh, 512 and
  1024 (dim 256 / 512 x 2 heads: the column loop);
  bf16: (1, 32, 256, 9) (2, 32, 256, 1) (2, 32, 256, 9) (1, 48, 256, 3) (2, 48, 128, 8) (1, 64, 64, 5) (2, 64, 256, 6), z / dz stored
  fp32 and bf16.
Meshes end inside their last slab (n_out = 2088 = 8 x 256 + 40: one whole pass, one of 8 rows, six skipped; 537 = 2 x 256 + 25 and
1305: a partial first pass), have sparse slabs beside full ones (nkeys 8 and 11 under um 32 and 48) and latent keys no row lists.

Not reachable through MeshPlan.fold_plan (listed, not forced):
* (rows 128 | 64, um 32): the plan builder takes the tallest slabs whose unions fit 64 keys, and two slabs of <= 32 keys each make
  a slab of twice the rows with <= 64 - such a pair always lands on the taller slabs;
* n_in < 96: MeshPlan builds candidate lists only where 3 x capacity <= n_in, and the smallest capacity is 32.  The 1024-wide
  fold_reduce_kernel case therefore has 128 latent points, not 64.

Thin tail: all of n1 in {64, 128, 256} x n2 in 1..4 x {erf, polynomial CDF} x z {fp32, bf16} at 997 / 333 / 211 rows (partial last
row group; 997 % 4 = 1 for the four-rows-per-pass n1 = 64), ld > width everywhere; 70 001 x 256 x 4 and 270 001 x 64 x 1 rows in fp32
(both grid caps bind: more than one trip of the U = 4 loop, the last one partial); gradients are ADDED to pre-filled tensors, the
scratch is left zero, a second call agrees to the atomics' order (1e-6).  Bounds: y 1e-6, dz and the weight gradients 1e-5 (the
whole-tensor bounds of tests/test_gpu_round6.py, here per block), a bf16-stored dz 2^-8; the polynomial-CDF instances add twice the
polynomial's own error, measured on the CPU against erf by `poly_cdf_error` (720 001 points of [-9, 9]): 2.3e-8.

Worst measured block per quantity (MI355X; every case meets its bound outright, none needs the wider
max(bound, 2 x the fp32 oracle's own distance) of tests/test_gpu_reductions.py and none is given it):
  pw 1.1e-7, qw 4.5e-7 (bound 2e-6); z 1.3e-7 (2e-6), bf16-stored z 2.1e-3 (2^-8 = 3.9e-3); d(VW) tiles 2.4e-7, atomics 2.3e-7
  (1e-5); d(c) 5.5e-7 in both forms (1e-4); tail y 2.4e-7 (1e-6), dz 1.2e-7 (1e-5), bf16-stored dz 2.5e-3 (3.9e-3), d_b1 9.8e-8,
  d_w2 8.9e-8, d_b2 1.7e-7 (1e-5).  The bf16-mode cases are within the same figures: with the operands rounded as the kernel rounds
  them nothing of the mode's 2e-2 is left.

What the suite found: fold_bwd_kernel kept wred[8] and keys_s[64] right behind its tiles, where the epilogue's exchange tile
overwrote them in the bf16 flavour with um = 32 (the only instances whose tiles are shorter than the exchange tile).  The atomic form
added every d(VW) row of a slab to key 0 and d(scale) could lose a wave's partial; before the fix test_fold_backward_atomics failed
for fold-bf16-h1-um32-r256-s9, fold-bf16-h2-um32-r256-s1 and fold-bf16-h2-um32-r256-s9 (the d(scale) race did not show in the tiles
form on the run that was made), with wred and keys_s behind the longer of the two layouts all pass.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pit_oracle as orc
from test_gpu_att_edges import GUARD, Buf, compare, lattice

pytestmark = pytest.mark.gpu

FP32, BF16 = 0, 1                                        # PIT_MATH_*
X16, OUT16, DOUT16 = 0x100, 0x800, 0x1000                # PIT_IO_X_BF16, _OUT_BF16, _DOUT_BF16
E_NULL, E_SIZE, E_UNSUPPORTED = -1, -2, -4               # PIT_ERR_*
SLOTS, EU = 1024, 64                                     # PIT_DSCALE_SLOTS, PIT_SLAB_UNION_MAX
TOL = dict(fwd=2e-6, dv=1e-5, dc=1e-4, z16=2.0 ** -8)
FILL64 = 0x7FF8DEADBEEF0000


def _lib_():
    from position_induced_transformer_amd import _lib
    return _lib


class DBuf:
    """n zeroed doubles between GUARD NaN-patterned doubles either side."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
        self.t = self.buf.view(torch.float64)[GUARD:GUARD + n]
        self.t.zero_()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        return bool((self.buf[:GUARD] == FILL64).all()) and bool((self.buf[GUARD + self.n:] == FILL64).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _synth(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# --------------------------------------------------------------------------- meshes and their fp64 weights (once per (mesh, heads))
def _line(n, lo, hi, seed):
    """n jittered lattice points of [lo, hi] in one dimension, in order."""
    return (lo + (hi - lo) * lattice(n, 1, seed)).contiguous()


# name -> (mesh_out, mesh_in, locality) and what fold_plan makes of it: (rows, max_union, n_slabs)
MESHES = {
    "line-u32-s9": (lambda: (_line(2088, 0.0, 1.0, 1), _line(128, 0.0, 1.0, 2), 0.05), (256, 24, 9)),
    "line-u32-s1": (lambda: (_line(217, 0.1, 0.3, 3), _line(128, 0.0, 1.0, 4), 0.03), (256, 30, 1)),
    "line-u48-s3": (lambda: (_line(537, 0.08, 0.58, 5), _line(128, 0.0, 1.0, 6), 0.05), (256, 38, 3)),
    "line-u48-r128": (lambda: (_line(1000, 0.0, 1.0, 7), _line(256, 0.0, 1.0, 8), 0.02), (128, 40, 8)),
    "line-u48-r64": (lambda: (_line(420, 0.0, 1.0, 19), _line(256, 0.0, 1.0, 20), 0.02), (64, 45, 7)),
    "line-u64-r256": (lambda: (_line(1305, 0.0, 1.0, 9), _line(256, 0.0, 1.0, 10), 0.02), (256, 57, 6)),
    "line-u64-r64": (lambda: (_line(300, 0.0, 1.0, 21), _line(256, 0.0, 1.0, 22), 0.02), (64, 61, 5)),
    "grid-u64-r128": (lambda: (lattice(900, 2, 13, 0.3), lattice(144, 2, 14, 0.3), 0.04), (128, 58, 8)),
}


@functools.lru_cache(maxsize=None)
def mesh_ref(name, H):
    """The pair's meshes, head scales c and the fp64 P_h, Q_h (H, n_out, n_in) of the operator's definition."""
    mo, mi, loc = MESHES[name][0]()
    n_in = mi.shape[0]
    m = orc.sqdist("euclid", mo, mi)                                     # fp32 (N, J)
    mk, mk1, mmin = orc.row_order_stats(m, loc)
    _, w = orc.quantile_rank(loc, n_in)
    cvec = (torch.tensor([1.7, 2.9][:H], dtype=torch.float32) * (3.0 / float(mk.median()))).float()      # c m_(k) of order 3 .. 5
    P, Q = [], []
    for h in range(H):
        s = m * cvec[h]                                                  # fp32: the operator's scores
        T = orc.lerp_threshold(mk * cvec[h], mk1 * cvec[h], w)
        smin = mmin * cvec[h]
        s64, t64 = s.double(), T[:, None].double()
        ulp = torch.exp2(torch.floor(torch.log2(t64.abs().clamp(min=1e-38))) - 23)
        assert bool(((s64 - t64).abs() > 4 * ulp).all()), "a score within 4 ulp of its threshold: choose another seed"
        a = torch.where(s <= T[:, None], torch.exp(smin[:, None].double() - s64), torch.zeros((), dtype=torch.float64))
        p = a / a.sum(-1, keepdim=True)
        mbar = (p * m.double()).sum(-1, keepdim=True)
        P.append(p)
        Q.append(p * (m.double() - mbar))
    return dict(mo=mo, mi=mi, loc=loc, cvec=cvec, P=torch.stack(P), Q=torch.stack(Q))


def evaluate(P, Q, vw, dz, H):
    """z (b, N, dim), d(VW) (b, J, dim * H) head-interleaved, d(c) (H) in fp64 from dense P, Q (H, N, J)."""
    b, J, hd = vw.shape
    VW = vw.double().view(b, J, hd // H, H)
    dz = dz.double()
    z = sum(torch.matmul(P[h], VW[..., h]) for h in range(H))
    dvw = torch.stack([torch.matmul(P[h].T, dz) for h in range(H)], -1).reshape(b, J, hd)
    dc = torch.stack([-(torch.matmul(Q[h], VW[..., h]) * dz).sum() for h in range(H)])
    return z, dvw, dc


def union_slots(max_union):
    return 32 if max_union <= 32 else (48 if max_union <= 48 else 64)


# --------------------------------------------------------------------------- the fold runner
class Fold:
    """One case: the plan (asserted), the guarded weight tiles (verified), and one method per entry call."""

    def __init__(self, mesh, H, bf, dim, batch, z16=False, dz16=False):
        from position_induced_transformer_amd import ops
        L = _lib_()
        self.H, self.bf, self.dim, self.b, self.z16, self.dz16 = H, bf, dim, batch, z16, dz16
        self.ref = ref = mesh_ref(mesh, H)
        self.plan = plan = ops.MeshPlan("euclid", ref["mo"].cuda(), ref["mi"].cuda(), ref["loc"], False)
        fp = plan.fold_plan()
        assert fp is not None, "no fold plan for this mesh pair"
        self.sp, self.mu, keep, self.mc = fp
        sp = self.sp
        self.keys, self.nkeys, self.rev_ptr, self.rev_ent = keep[2].cpu().long(), keep[3].cpu().long(), keep[4], keep[5]
        print(f"  plan: rows {sp.rows}, max_union {self.mu}, n_slabs {sp.n_slabs}, nkeys {self.nkeys.tolist()}, longest list {self.mc}")
        assert (sp.rows, self.mu, sp.n_slabs) == MESHES[mesh][1]
        self.um = um = union_slots(self.mu)
        assert int(self.nkeys.max()) == self.mu
        self.n_out, self.n_in, self.rows, self.ns = plan.n_out, plan.n_in, sp.rows, sp.n_slabs
        assert self.n_out % 32 not in (0, 16) and self.ns == -(-self.n_out // self.rows)
        listed = torch.zeros(self.n_in, dtype=torch.bool)
        for s in range(self.ns):
            listed[self.keys[s, :int(self.nkeys[s])]] = True
        self.unlisted = ~listed
        rp = self.rev_ptr.cpu()
        assert torch.equal((rp[1:] - rp[:-1]) == 0, self.unlisted)
        # ---- the weight tiles
        nt = self.ns * H * self.rows
        self.pw, self.qw = Buf(1, nt, um), Buf(1, nt, um)
        self.pw16, self.qw16 = (Buf(1, nt, um, bf16=True), Buf(1, nt, um, bf16=True)) if bf else (None, None)
        self.head, self.scale = Buf(1, 1, H, data=ref["cvec"]), Buf(1, 1, H)
        rc = L.lib().pit_fold_weights(ctypes.byref(sp), self.head.ptr, 1, H, self.mu, self.mc, self.pw.ptr, self.qw.ptr, self.scale.ptr,
                                      self.pw16.ptr if bf else None, self.qw16.ptr if bf else None, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert self.head.untouched() and torch.equal(self.scale.cpu().view(-1), ref["cvec"])
        wantp, wantq, live = self.tiles_of(ref["P"]), self.tiles_of(ref["Q"]), self.tiles_of(torch.ones_like(ref["P"])) > 0
        for name, buf, want in (("pw", self.pw, wantp), ("qw", self.qw, wantq)):
            assert buf.untouched() and self.scale.untouched()
            got = buf.cpu()
            compare(name, got, want.view(1, nt, um), TOL["fwd"])
            assert bool((got.view(-1, self.rows, um)[~live] == 0).all()), f"{name}: slots beyond the union / rows beyond n_out are not 0"
        if bf:
            for name, b16, b32 in (("pw16", self.pw16, self.pw), ("qw16", self.qw16, self.qw)):
                assert b16.untouched()
                assert torch.equal(bits(b16.t), bits(b32.t.bfloat16())), f"{name} is not {name[:2]}.bfloat16() bit for bit"
            # the operands as the bf16 flavour reads them: dense P, Q from the bf16 tiles
            self.P, self.Q = self.dense_of(self.pw16.cpu().double()), self.dense_of(self.qw16.cpu().double())
        else:
            self.P, self.Q = ref["P"], ref["Q"]
        # ---- operands and the reference
        rnd = (lambda t: t.bfloat16().float())
        vw = _synth((batch, self.n_in, H * dim), 31)
        dz = _synth((batch, self.n_out, dim), 32)
        if dz16:
            dz = rnd(dz)
        self.vw = Buf(batch, self.n_in, H * dim, 4, 3, data=vw)
        self.dz = Buf(batch, self.n_out, dim, 8, 2, bf16=dz16, data=dz)
        self.z64, self.dvw64, self.dc64 = evaluate(self.P, self.Q, rnd(vw) if bf else vw, rnd(dz) if bf else dz, H)
        self.mode = BF16 if bf else FP32
        self.wp, self.wq = ((self.pw16, self.qw16) if bf else (self.pw, self.qw))

    def tiles_of(self, D):
        """(n_slabs * H, rows, um) tiles of a dense (H, N, J) tensor: slot -> keys[s, slot], 0 beyond nkeys[s] and beyond n_out."""
        out = torch.zeros(self.ns * self.H, self.rows, self.um, dtype=torch.float64)
        for s in range(self.ns):
            nk, r1 = int(self.nkeys[s]), min(self.n_out - s * self.rows, self.rows)
            for h in range(self.H):
                out[s * self.H + h, :r1, :nk] = D[h, s * self.rows:s * self.rows + r1][:, self.keys[s, :nk]]
        return out

    def dense_of(self, tiles):
        tiles = tiles.view(self.ns * self.H, self.rows, self.um)
        D = torch.zeros(self.H, self.n_out, self.n_in, dtype=torch.float64)
        for s in range(self.ns):
            nk, r1 = int(self.nkeys[s]), min(self.n_out - s * self.rows, self.rows)
            for h in range(self.H):
                D[h, s * self.rows:s * self.rows + r1, self.keys[s, :nk]] = tiles[s * self.H + h, :r1, :nk]
        return D

    def inputs_untouched(self):
        return all(t.untouched() for t in (self.vw, self.dz, self.pw, self.qw) + ((self.pw16, self.qw16) if self.bf else ()))

    def forward(self, rc_want=0, sp=None, H=None, dim=None, mu=None, vw=None, z=None, ld_z=None):
        L = _lib_()
        vw = vw or self.vw
        z = z or Buf(self.b, self.n_out, self.dim, 4, 3, bf16=self.z16)
        rc = L.lib().pit_fold_att_fwd(ctypes.byref(sp or self.sp), vw.ptr, vw.ld, vw.bs, self.b, H or self.H, dim or self.dim, self.wp.ptr,
                                      z.ptr, ld_z or z.ld, z.bs, self.mu if mu is None else mu,
                                      self.mode | (OUT16 if self.z16 else 0), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == rc_want, rc
        assert self.inputs_untouched()
        if rc:
            assert z.unwritten()
            return
        assert z.untouched()
        compare("z (bf16-stored)" if self.z16 else "z", z.cpu(), self.z64, TOL["z16"] if self.z16 else TOL["fwd"])

    def backward(self, tiles, want_dv=True, want_dc=True, rc_want=0, rev=True, mu=None, numeric=True):
        """The tiles form writes d_vw (NaN before), the atomic form adds to it (a known tensor before).  Returns the d_vw bits."""
        L = _lib_()
        hd = self.H * self.dim
        pre = None
        if want_dv and not tiles:
            pre = 0.5 * _synth((self.b, self.n_in, hd), 33)
            pre[:, self.unlisted, ::3] = -0.0
        dvw = Buf(self.b, self.n_in, hd, 4, 2, data=pre) if want_dv else None
        tb = Buf(1, self.b * self.ns * EU, hd) if tiles else None
        ds = DBuf(self.H * SLOTS) if want_dc else None
        rc = L.lib().pit_fold_att_bwd(ctypes.byref(self.sp), self.vw.ptr, self.vw.ld, self.vw.bs, self.b, self.H, self.dim,
                                      self.wp.ptr, self.wq.ptr, self.dz.ptr, self.dz.ld, self.dz.bs,
                                      dvw.ptr if dvw else None, dvw.ld if dvw else 0, dvw.bs if dvw else 0, ds.ptr if ds else None,
                                      tb.ptr if tb else None, self.rev_ptr.data_ptr() if rev else None,
                                      self.rev_ent.data_ptr() if rev else None, self.mu if mu is None else mu,
                                      self.mode | (DOUT16 if self.dz16 else 0), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == rc_want, rc
        assert self.inputs_untouched()
        if rc:
            assert (tb is None or tb.unwritten()) and (ds is None or float(ds.t.abs().max()) == 0.0)
            assert dvw is None or (dvw.unwritten() if pre is None else torch.equal(bits(dvw.t.cpu()), bits(pre)))
            return None
        form = "tiles" if tiles else "atomics"
        assert tb is None or tb.untouched()
        got = None
        if dvw is not None:
            assert dvw.untouched()
            got = dvw.t.cpu()
            if numeric:
                compare(f"d(VW) {form}", got, self.dvw64 if tiles else self.dvw64 + pre.double(), TOL["dv"])
            want0 = torch.zeros_like(got) if tiles else pre
            assert torch.equal(bits(got[:, self.unlisted]), bits(want0[:, self.unlisted])), "the row of a key that no slab holds changed"
        if ds is not None:
            assert ds.untouched()
            slots = ds.t.cpu().view(self.H, SLOTS)
            assert bool(torch.isfinite(slots).all())
            if numeric:
                compare(f"d(c) {form}", slots.sum(1).view(1, 1, -1), self.dc64.view(1, 1, -1), TOL["dc"], 1, 1)
            return got, slots
        return got, None


@functools.lru_cache(maxsize=None)
def fold(case):
    return Fold(*case)


def _f(id_, *case):
    return pytest.param(case, id=id_)


# (mesh, heads, bf16 math, dim, batch, z bf16-stored, dz bf16-stored)
FOLD = [
    _f("fold-fp32-h1-um32-r256-s9", "line-u32-s9", 1, False, 64, 3),
    _f("fold-fp32-h2-um32-r256-s1", "line-u32-s1", 2, False, 128, 1),
    _f("fold-fp32-h1-um48-r256-s3", "line-u48-s3", 1, False, 128, 2),
    _f("fold-fp32-h2-um48-r128-s8", "line-u48-r128", 2, False, 64, 3),
    _f("fold-fp32-h1-um64-r64-s5", "line-u64-r64", 1, False, 64, 2),
    _f("fold-fp32-h2-um64-r256-s6", "line-u64-r256", 2, False, 128, 2),
    _f("fold-fp32-h2-um48-r64-s7-io16", "line-u48-r64", 2, False, 64, 1, True, True),
    _f("fold-fp32-h2-um64-r128-s8-grid", "grid-u64-r128", 2, False, 64, 2),
    _f("fold-fp32-h2-um32-r256-s1-w512", "line-u32-s1", 2, False, 256, 1),
    _f("fold-fp32-h2-um32-r256-s1-w1024", "line-u32-s1", 2, False, 512, 1),
    _f("fold-bf16-h1-um32-r256-s9", "line-u32-s9", 1, True, 64, 3, True, True),
    _f("fold-bf16-h2-um32-r256-s1", "line-u32-s1", 2, True, 128, 1),
    _f("fold-bf16-h2-um32-r256-s9", "line-u32-s9", 2, True, 64, 2, True, True),
    _f("fold-bf16-h1-um48-r256-s3", "line-u48-s3", 1, True, 128, 2, True, False),
    _f("fold-bf16-h2-um48-r128-s8", "line-u48-r128", 2, True, 64, 3, False, True),
    _f("fold-bf16-h1-um64-r64-s5", "line-u64-r64", 1, True, 64, 2),
    _f("fold-bf16-h2-um64-r256-s6", "line-u64-r256", 2, True, 128, 2, True, True),
]


@pytest.mark.parametrize("case", FOLD)
def test_fold_weights_and_forward(case):
    """pit_fold_weights' tiles (checked when the case is set up) and pit_fold_att_fwd."""
    fold(case).forward()


@pytest.mark.parametrize("case", FOLD)
def test_fold_backward_tiles(case):
    """Per-slab tiles + fold_reduce_kernel: d(VW) and d(c); the same bits on a second call; d(VW) alone gives the same bits as the
    full call."""
    f = fold(case)
    a, _ = f.backward(True)
    b, _ = f.backward(True)
    assert torch.equal(bits(a), bits(b)), "the tiles form is not reproducible"
    c, none = f.backward(True, want_dc=False)
    assert none is None and torch.equal(bits(a), bits(c)), "d(VW) alone differs from the full call's"


@pytest.mark.parametrize("case", FOLD)
def test_fold_backward_atomics(case):
    """tiles = nullptr: fp32 atomic adds into a pre-filled d_vw, d(c) from the same launch; then d(scale) alone (d_vw = nullptr),
    whose slots agree with the full call's to the fp64 atomics' order, and d(VW) alone (dscale = nullptr)."""
    f = fold(case)
    _, full = f.backward(False)
    _, alone = f.backward(False, want_dv=False)
    assert float((alone.sum(1) - full.sum(1)).abs().max()) <= 1e-10 * float(full.abs().sum(1).max())
    f.backward(False, want_dc=False)


def test_fold_refusals():
    """Arguments the entries refuse: the code as pit_fold.hip returns it, nothing written."""
    f = fold(FOLD[1].values[0])
    sp16, patch = type(f.sp).from_buffer_copy(f.sp), type(f.sp).from_buffer_copy(f.sp)
    sp16.rows, patch.patch_w = 16, 4
    hd = f.H * f.dim
    for kw, rc in ((dict(H=3), E_UNSUPPORTED), (dict(dim=96), E_UNSUPPORTED), (dict(mu=0), E_UNSUPPORTED), (dict(mu=65), E_UNSUPPORTED),
                   (dict(vw=Buf(f.b, f.n_in, hd, 5, 3)), E_SIZE), (dict(z=Buf(f.b, f.n_out, f.dim, 4, 3, off=1)), E_SIZE),
                   (dict(ld_z=f.dim - 4), E_SIZE), (dict(sp=sp16), E_NULL), (dict(sp=patch), E_NULL)):
        f.forward(rc_want=rc, **kw)
    f.backward(True, rc_want=E_NULL, rev=False)                       # tiles without rev_ptr
    f.backward(True, rc_want=E_UNSUPPORTED, mu=65)
    f.backward(False, rc_want=E_UNSUPPORTED, mu=0)


# --------------------------------------------------------------------------- thin tail
@functools.lru_cache(maxsize=1)
def poly_cdf_error():
    """max |normal_cdf_fast - Phi| over [-9, 9]: the polynomial of csrc/pit_common.h with its fp32 coefficients, evaluated in fp64 (its
    own error; the fp32 rounding of its evaluation is what the fp32 bounds already allow for erff)."""
    f = lambda v: float(np.float32(v))
    x = np.linspace(-9.0, 9.0, 720001)
    t = 1.0 / (np.abs(x) * f(0.28284271247) + 1.0)
    e = np.exp2(x * x * f(-0.72134752044))
    p = np.full_like(x, f(-0.100061134))
    for c in (0.354291141, -0.184991121, 0.233760774, 0.0810635462, 0.115936771):
        p = p * t + f(c)
    q = p * t * e
    cdf = np.where(x > 0, 1.0 - q, q)
    exact = 0.5 * (1.0 + torch.erf(torch.from_numpy(x) / 2.0 ** 0.5)).numpy()
    return float(np.abs(cdf - exact).max())


class Tail:
    def __init__(self, rows, n1, n2, bf, z16, seed=5):
        self.rows, self.n1, self.n2, self.bf, self.z16 = rows, n1, n2, bf, z16
        g = torch.Generator().manual_seed(seed + n1 + n2)
        z = torch.randn(1, rows, n1, generator=g)
        if z16:
            z = z.bfloat16().float()
        b1, w2 = torch.randn(n1, generator=g), torch.randn(n2, n1, generator=g) / n1 ** 0.5
        # (d_y with a mean: d_b2 = sum d_y is then no cancelling sum, whose fp32 rounding - and the order of its atomics - would be
        # measured against a result of arbitrary smallness; for n2 = 1 it is the only element of its tensor)
        b2, dy = torch.randn(n2, generator=g), 0.5 + torch.randn(1, rows, n2, generator=g)
        self.z, self.b1, self.w2 = Buf(1, rows, n1, 4, bf16=z16, data=z), Buf(1, 1, n1, data=b1), Buf(1, n2, n1, data=w2)
        self.b2, self.dy = Buf(1, 1, n2, data=b2), Buf(1, rows, n2, 1, data=dy)
        t = z[0].double() + b1.double()
        cdf = 0.5 * (1.0 + torch.erf(t / 2.0 ** 0.5))
        a = t * cdf
        gp = cdf + t * torch.exp(-0.5 * t * t) / (2.0 * torch.pi) ** 0.5
        self.y64 = (a @ w2.double().T + b2.double())[None]
        dz = (dy[0].double() @ w2.double()) * gp
        self.dz64, self.db1, self.dw2, self.db2 = dz[None], dz.sum(0), dy[0].double().T @ a, dy[0].double().sum(0)
        self.mode = (BF16 if bf else FP32) | (X16 if z16 else 0)
        self.extra = 2.0 * poly_cdf_error() if bf else 0.0
        self.scratch = Buf(1, 1, _lib_().lib().pit_thin_tail_scratch_floats())
        self.scratch.t.zero_()

    def inputs_untouched(self):
        return all(t.untouched() for t in (self.z, self.b1, self.w2, self.b2, self.dy))

    def forward(self):
        L = _lib_()
        y = Buf(1, self.rows, self.n2, 3)
        rc = L.lib().pit_thin_tail_fwd(self.z.ptr, self.z.ld, self.rows, self.n1, self.n2, self.b1.ptr, self.w2.ptr, self.b2.ptr,
                                       y.ptr, y.ld, self.mode, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert self.inputs_untouched() and y.untouched()
        compare("tail y", y.cpu(), self.y64, 1e-6 + self.extra)

    def backward(self):
        L = _lib_()
        pre = [0.5 * _synth(s, 40 + i) for i, s in enumerate(((1, 1, self.n1), (1, self.n2, self.n1), (1, 1, self.n2)))]
        runs = []
        for _ in range(2):
            dz = Buf(1, self.rows, self.n1, 8, bf16=self.z16)
            g = [Buf(*p.shape, data=p) for p in pre]
            rc = L.lib().pit_thin_tail_bwd(self.z.ptr, self.z.ld, self.rows, self.n1, self.n2, self.b1.ptr, self.w2.ptr, self.dy.ptr,
                                           self.dy.ld, dz.ptr, dz.ld, g[0].ptr, g[1].ptr, g[2].ptr, self.scratch.ptr, self.mode,
                                           L.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0
            assert self.inputs_untouched() and dz.untouched() and all(t.untouched() for t in g) and self.scratch.untouched()
            assert float(self.scratch.t.abs().max()) == 0.0, "the scratch is not left zero"
            runs.append([dz.cpu()] + [t.cpu() for t in g])
        dz, db1, dw2, db2 = runs[0]
        compare("tail dz (bf16-stored)" if self.z16 else "tail dz", dz, self.dz64, (TOL["z16"] if self.z16 else 1e-5) + self.extra)
        compare("tail d_b1", db1, self.db1.view(1, 1, -1) + pre[0].double(), 1e-5 + self.extra)
        compare("tail d_w2", dw2, self.dw2[None] + pre[1].double(), 1e-5 + self.extra)
        compare("tail d_b2", db2, self.db2.view(1, 1, -1) + pre[2].double(), 1e-5 + self.extra)
        assert torch.equal(bits(runs[0][0]), bits(runs[1][0])), "dz differs between two calls"
        for u, v in zip(runs[0][1:], runs[1][1:]):
            assert float((u - v).norm()) <= 1e-6 * float(u.norm())


TAIL_ROWS = {64: 997, 128: 333, 256: 211}


@pytest.mark.parametrize("z16", [False, True], ids=["z32", "z16"])
@pytest.mark.parametrize("bf", [False, True], ids=["erf", "poly"])
@pytest.mark.parametrize("n2", [1, 2, 3, 4])
@pytest.mark.parametrize("n1", [64, 128, 256])
def test_tail_instances(n1, n2, bf, z16):
    """thin_tail_fwd / _bwd_kernel<N2 = 1 | 4, FAST, Z16> at every (n1, n2): tail-n1-n2-cdf-z."""
    t = Tail(TAIL_ROWS[n1], n1, n2, bf, z16)
    t.forward()
    t.backward()


@pytest.mark.parametrize("rows,n1,n2", [(70001, 256, 4), (270001, 64, 1)], ids=["tail-large-256x4", "tail-large-64x1"])
def test_tail_beyond_the_grid_caps(rows, n1, n2):
    """4096 forward / 2048 backward workgroups do not cover the rows: every wavefront makes more than one trip of its U = 4 loop and
    the last trip is partial."""
    rpw = 64 // (n1 // 4)
    assert rows > 4096 * 16 * rpw and rows > 2048 * 32 * rpw
    t = Tail(rows, n1, n2, False, False)
    t.forward()
    t.backward()


def test_tail_refusals():
    """Argument checks of tail_fill and the entries: nothing written."""
    L = _lib_()
    rows, n1, n2 = 37, 64, 2
    t = Tail(rows, n1, n2, False, False)
    zoff = Buf(1, rows, n1, 4, off=1)
    big = ((1 << 31) - 65536) // (4 * 256)
    # (z, ldz, rows, n1, n2) -> code
    bad = [((t.z, t.z.ld, rows, 96, n2), E_UNSUPPORTED), ((t.z, t.z.ld, rows, n1, 0), E_UNSUPPORTED), ((t.z, t.z.ld, rows, n1, 5), E_UNSUPPORTED),
           ((t.z, n1 - 4, rows, n1, n2), E_UNSUPPORTED), ((t.z, n1 + 2, rows, n1, n2), E_UNSUPPORTED), ((zoff, zoff.ld, rows, n1, n2), E_SIZE),
           ((t.z, 256, big, 256, n2), E_UNSUPPORTED)]
    for (z, ldz, r, a1, a2), want in bad:
        y, dz = Buf(1, rows, 4, 3), Buf(1, rows, n1, 8)
        g = [Buf(1, 1, n1), Buf(1, 4, n1), Buf(1, 1, 4)]
        rc = L.lib().pit_thin_tail_fwd(z.ptr, ldz, r, a1, a2, t.b1.ptr, t.w2.ptr, t.b2.ptr, y.ptr, y.ld, FP32, L.stream_ptr())
        assert rc == want, (rc, want, ldz, r, a1, a2)
        rc = L.lib().pit_thin_tail_bwd(z.ptr, ldz, r, a1, a2, t.b1.ptr, t.w2.ptr, t.dy.ptr, t.dy.ld, dz.ptr, dz.ld, g[0].ptr, g[1].ptr,
                                       g[2].ptr, t.scratch.ptr, FP32, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want, (rc, want, ldz, r, a1, a2)
        assert y.unwritten() and dz.unwritten() and all(b.unwritten() for b in g) and float(t.scratch.t.abs().max()) == 0.0
