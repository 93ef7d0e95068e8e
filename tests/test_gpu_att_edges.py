"""The candidate-list and union-tile kernels of the masked layers (csrc/pit_posatt.hip: posatt_sparse_rows / _rows_x / _cols / _cols_x /
_bwd_kernel / _overflow_cols / _rows8 / _cols8, posatt_union_kernel / _union_dv_kernel) one dispatch instance at a time, through the
raw C ABI: pit_posatt_fwd_job and pit_posatt_bwd.  The plan (statistics, candidate lists, their transpose) comes from ops.MeshPlan
and is an input here - the selection and list kernels have their own suite (tests/test_gpu_selection.py).

Every GPU case

* resets the library's launch record (pit_debug_att_counts, include/pit_hip.h), runs ONE entry and asserts the exact record: kind ->
  number of launches, and the PIT_ATT_LAST_* slots (template arguments, column blocks).  The expectation is written into the case
  (`rows=(NH, CR, grid.y)`, `cols=(CR, grid.y)`, `pair=(NH, CRR, CRC)`, `union=(NH, EPL, per)`), never re-derived from cr_for;
* hands every tensor the entry reads or writes as a view inside an allocation pre-filled with a NaN bit pattern (`Buf`): 64 guard
  rows before and after it, padding columns between rows (ld > width), padding rows between samples.  After the call every word
  outside an output's view still holds the pattern, every payload element is finite, and an input's NaN padding that leaks into a
  sum turns the result NaN;
* compares with an fp64 evaluation on the CPU.  The keep mask is the operator's definition (oracle/pit_oracle.py: fp32 squared
  distances, row_order_stats, the fp32 product with the injected scale c, the fp32 lerp); softmax weights, out, 1/L, mbar,
  d(values) and d(c) are fp64.  Outputs are compared PER BLOCK of 4 rows x 64 columns (one workgroup's rows, one lane-column
  group): rel-L2 of the block with the tensor's RMS as the floor of the denominator; 1/L and mbar per row; T and S_min bit for bit.
  Bounds per block: forward, 1/L, mbar 2e-6, d(values) 1e-5, d(c) 1e-4 (tests/test_gpu_ops.py); with a bf16-stored out / d_out 1e-2,
  1e-2, 5e-2 (tests/test_gpu_round5.py).  Every block of every case meets these bounds outright (the worst measured: forward
  3.8e-7, 1/L 1.9e-7, mbar 2.7e-7, d(values) 8.4e-7, d(c) 3.0e-6; bf16-stored out 2.6e-3), so no case needs the wider
  max(bound, 2 x the fp32 oracle's own distance) of tests/test_gpu_reductions.py and none is given it;
* asserts on the reference alone: no (row, key, head) has its fp32 score within 4 ulp of its fp32 threshold unless the score IS the
  threshold because m_(k) == m_(k+1) (duplicated keys: the lerp of equal ends is exact and 0 * c == 0 in any order), so no
  arithmetic order can flip the mask - given that the kernel forms the same fp32 distance bits for those keys as the selection
  kernel did (both 0.0f on a duplicated point; otherwise equal keys give equal bits in one kernel), so a failure of such a case is to
  be read as a flipped mask, not as a numeric regression; `overflow` cases have a row over the list capacity and one at or under it, all others none.

Case ids: ``list-*`` the rows / cols instances by (NH, CR); ``x-*`` the XCD-remapped twins (grid.y >= 16) and the case just under
the switch; ``pair-*`` the merged backward by (CRR, CRC), its decline and the bf16 d_out forms, ``cols-d16-*``
d(values) alone on the bf16 d_out instances; ``tail-*`` list lengths and gather
group tails; ``over-*`` overflowed rows; ``coord-*`` coordinate channels, ``copy-*`` the concat form; ``union-*`` the union
tiles; ``decl-*`` shapes the union form declines (the list kernels run, the result is still right); ``wide-*`` 4..8 coordinates;
``lmda-*`` the head handed over as lmda (scale_out, PIT_ATT_HEAD_SCALE); the rider tests assert the record and the attention result
of posatt_sparse_rows_w / _rows_dw / _bwd_dw_kernel and bracket their size limits (the carried GEMMs are tests/test_gpu_riders.py's).

Instances the default dispatch cannot reach (listed, not forced):

* ``posatt_sparse_bwd_dw_kernel<NH, 8, *>``: not instantiated - launch_sparse_bwd_pair carries a rider at crr <= 4 only;
* ``posatt_sparse_cols<1, true>``: bf16 d_out walks column pairs, launch_sparse_cols takes max(2, cr) (static_assert in the body);
* the `xtotal < 2^31` guard of both remaps: 8 * grid.x * ceil(grid.y / 8) >= 2^31 needs more than 2^28 row groups.
"""
import functools

import pytest
import torch

import pit_oracle as orc

pytestmark = pytest.mark.gpu

FILL32, FILL16 = 0x7FC0BEEF, 0x7FC1          # quiet NaNs (fp32 / bf16) with a recognisable payload
GUARD = 64
FP32, BF16 = 0, 1                           # PIT_MATH_*
OUT16, DOUT16, UNION = 0x800, 0x1000, 0x2000
UNSUPPORTED = -4                            # PIT_ERR_UNSUPPORTED
TOL = {False: dict(fwd=2e-6, dv=1e-5, dc=1e-4), True: dict(fwd=1e-2, dv=1e-2, dc=5e-2)}   # key: bf16 storage involved

KINDS = ("list_rows_fwd", "list_rows_dscale", "list_rows_x", "list_rows_w", "list_rows_dw", "list_cols", "list_cols_x", "list_cols_d16",
         "list_pair", "list_pair_dw", "list_pair_d16", "list_overflow", "list_rows8", "list_cols8", "list_overflow8", "union_fwd",
         "union_dscale", "union_dv", "union_zero", "dhead_finish", "head_scale", "dense", "last_rows", "last_cols", "last_pair",
         "last_union", "last_union_per", "last_grid_y")          # PIT_ATT_* in order


def counts(reset=True):
    from position_induced_transformer_amd import ops
    c = ops.att_launch_counts(reset=reset)
    assert len(c) == len(KINDS)
    return {k: v for k, v in zip(KINDS, c) if v}


# --------------------------------------------------------------------------- guard bands
class Buf:
    """A (b, rows, n) view - fp32 or bf16 - with row pitch n + pad and `gap` padding rows between samples, `off` elements off the
    start, inside one allocation filled with the NaN pattern: GUARD rows before and after it.  `data` makes it an input."""

    def __init__(self, b, rows, n, pad=0, gap=0, off=0, bf16=False, data=None):
        self.shape, self.ld, self.fill = (b, rows, n), n + pad, FILL16 if bf16 else FILL32
        self.bs = (rows + gap) * self.ld
        self.strides, self.start = (self.bs, self.ld, 1), GUARD * self.ld + off
        total = (2 * GUARD + b * (rows + gap)) * self.ld + off + 8
        self.buf = torch.full((total,), self.fill, dtype=torch.int16 if bf16 else torch.int32, device="cuda")
        self.t = self.buf.view(torch.bfloat16 if bf16 else torch.float32).as_strided(self.shape, self.strides, self.start)
        if data is not None:
            self.t.copy_(data.reshape(self.shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        c = self.buf.clone()
        c.as_strided(self.shape, self.strides, self.start).fill_(self.fill)
        return bool((c == self.fill).all())

    def unwritten(self):
        return bool((self.buf == self.fill).all())

    def cpu(self):
        return self.t.float().cpu()


# --------------------------------------------------------------------------- block-wise comparison (CPU, fp64)
def block_errs(got, ref, br=4, bc=64):
    """(b, row blocks, column blocks) of ||got - ref||_block / max(||ref||_block, rms(ref) sqrt(block size)) for (b, r, c) tensors; partial
    blocks at the edges count as blocks of their own.  A non-finite `got` gives inf everywhere."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return torch.full((1, 1, 1), float("inf"), dtype=torch.float64)
    b, r, c = ref.shape
    rb, cb = (r + br - 1) // br, (c + bc - 1) // bc

    def sums(t):
        p = torch.zeros(b, rb * br, cb * bc, dtype=torch.float64)
        p[:, :r, :c] = t
        return p.view(b, rb, br, cb, bc).sum(dim=(2, 4))
    num, den = sums((got - ref) ** 2), sums(ref ** 2)
    rows_in = torch.clamp(r - br * torch.arange(rb), max=br).double()
    cols_in = torch.clamp(c - bc * torch.arange(cb), max=bc).double()
    floor = torch.clamp(rows_in[:, None] * cols_in[None, :] * float((ref ** 2).mean()), min=1e-300)
    return torch.sqrt(num / torch.maximum(den, floor[None]))


def compare(name, got, ref64, bound, br=4, bc=64):
    """Every block of `got` within `bound` of the fp64 reference.  Prints before it asserts."""
    e = block_errs(got, ref64, br, bc)
    print(f"  {name}: worst block {float(e.max()):.3e} (bound {bound:.0e})")
    assert bool(torch.isfinite(e).all()), f"{name}: NaN or inf in the payload"
    bad = e > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} blocks over the bound, worst {float(e.max()):.3e} > {bound:.0e}"


# --------------------------------------------------------------------------- meshes and references (once per case, never modified)
def lattice(n, sdim, seed, jitter=0.3):
    """n points: a row-major lattice on the unit cube, coherently ordered, jittered by `jitter` of the spacing, cut to n points."""
    g = torch.Generator().manual_seed(seed)
    side = 2
    while side ** sdim < n:
        side += 1
    axes = [torch.linspace(0, 1, side)] * sdim
    mesh = torch.stack([t.reshape(-1) for t in torch.meshgrid(*axes, indexing="ij")], -1)[:n].clone()
    mesh += (2.0 * torch.rand(mesh.shape, generator=g) - 1.0) * jitter / (side - 1)
    return mesh.contiguous()


def _synth(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _evaluate(m, c, T, smin, V, dout, col0, dtype):
    """out (b, N, H*D), 1/L and mbar (mb, H, N), d(values) (b, J, D), d(c) (H) from the fp32 mask quantities, arithmetic in `dtype` (fp64)."""
    H, D = c.numel(), V.shape[-1]
    V = V.to(dtype)
    outs, invl, mbar, dv, dc = [], [], [], torch.zeros(V.shape, dtype=dtype), []
    for h in range(H):
        s = m * c[h]                                                    # fp32: the operator's scores
        keep = s <= T[:, h, :, None]
        a = torch.where(keep, torch.exp((smin[:, h, :, None].to(dtype) - s.to(dtype))), torch.zeros((), dtype=dtype))
        L = a.sum(-1)
        P = a / L[..., None]
        mb_ = (P * m.to(dtype)).sum(-1)
        outs.append(torch.matmul(P, V))
        invl.append(1.0 / L)
        mbar.append(mb_)
        if dout is not None:
            g = dout[..., col0 + h * D: col0 + (h + 1) * D].to(dtype)
            dv += torch.matmul(P.transpose(-1, -2), g)
            Q = P * (m.to(dtype) - mb_[..., None])
            dc.append(-(g * torch.matmul(Q, V)).sum())
    res = dict(out=torch.cat(outs, -1), invl=torch.stack(invl, 1), mbar=torch.stack(mbar, 1), dv=dv)
    if dout is not None:
        res["dc"] = torch.stack(dc)
    return res


@functools.lru_cache(maxsize=2)
def reference(key):
    """Inputs and references of one case.  `key` = the hashable geometry of the case (see CASES)."""
    c = dict(key)
    n_out, n_in, b, dim, H, sdim = c["n_out"], c["n_in"], c["batch"], c["dim"], c["heads"], c.get("sdim", 2)
    per_sample, cd, loc, seed = c.get("per_sample", False), c.get("cd", 0), c["loc"], c.get("seed", 1)
    self_attn = c.get("copy", False)
    mb = b if per_sample else 1

    def one(i):
        if c.get("cloud"):
            g = torch.Generator().manual_seed(100 * seed + i)
            mi_, mo_ = torch.rand(n_in, sdim, generator=g), torch.rand(n_out, sdim, generator=g)
        else:
            mi_ = lattice(n_in, sdim, 100 * seed + i)
            mo_ = mi_ if self_attn else lattice(n_out, sdim, 100 * seed + 50 + i, jitter=0.35)
        if c.get("shuffle"):                                            # incoherent row order: big unions per tile
            mo_ = mo_[torch.randperm(n_out, generator=torch.Generator().manual_seed(seed))]
        dup, rows_dup = c.get("dup", (0, 0))
        if dup:                                                         # duplicated keys and the rows sitting on them
            mi_ = mi_.clone()
            mo_ = mo_.clone()
            mi_[:dup] = mi_[:1]
            at = c.get("dup_at", 0)
            mo_[at:at + rows_dup] = mi_[:1]
        return mo_.contiguous(), mi_.contiguous()
    pairs = [one(i) for i in range(mb)]
    mo, mi = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])           # (mb, N, s), (mb, J, s)
    vals = _synth((b, n_in, dim - cd), 7 * seed + 1)
    cvec = torch.tensor([1.7, 2.9, 2.2, 1.3][:H], dtype=torch.float32) * float(c.get("cmul", 30.0))
    width = c.get("col0", dim if self_attn else 0) + H * dim
    dout = _synth((b, n_out, width), 7 * seed + 2)
    if c.get("dout16"):
        dout = dout.bfloat16().float()
    V = vals if cd == 0 else torch.cat((mi[..., :cd].expand(b, -1, -1), vals), -1)
    m = orc.sqdist("euclid", mo, mi)                                    # fp32 (mb, N, J)
    mk, mk1, mmin = orc.row_order_stats(m, loc)
    _, w = orc.quantile_rank(loc, n_in)
    T = torch.stack([orc.lerp_threshold(mk * cvec[h], mk1 * cvec[h], w) for h in range(H)], 1)     # (mb, H, N) fp32
    smin = torch.stack([mmin * cvec[h] for h in range(H)], 1)
    kept = torch.zeros(mb, n_out, dtype=torch.long)
    for h in range(H):                                                  # the 4-ulp condition (module docstring)
        s, t = (m * cvec[h]).double(), T[:, h, :, None].double()
        ulp = torch.exp2(torch.floor(torch.log2(t.abs().clamp(min=1e-38))) - 23)
        dist = (s - t).abs()
        exact_tie = (dist == 0) & (mk == mk1)[..., None]
        assert bool(((dist > 4 * ulp) | exact_tie).all()), "a score within 4 ulp of its threshold: choose another seed"
        kept = torch.maximum(kept, (s <= t).sum(-1))
    col0 = c.get("col0", dim if self_attn else 0)
    r64 = _evaluate(m, cvec, T, smin, V, dout, col0, torch.float64)
    r64["dv"] = r64["dv"][..., cd:]
    if self_attn and cd == 0:
        r64["dv"] = r64["dv"] + dout[..., :dim].double()                # add_residual
    return dict(mo=mo, mi=mi, vals=vals, cvec=cvec, dout=dout, T=T, smin=smin, kept=kept, r64=r64, w=w)


# --------------------------------------------------------------------------- the runner
def _lib_():
    from position_induced_transformer_amd import _lib
    return _lib


class Run:
    """One case on the GPU: the plan, the guarded inputs, and one method per entry call."""

    def __init__(self, c):
        from position_induced_transformer_amd import ops
        self.c = c
        geo = tuple(sorted((k, v) for k, v in c.items() if k in GEOMETRY))
        self.ref = ref = reference(geo)
        self.b, self.dim, self.H, self.cd = c["batch"], c["dim"], c["heads"], c.get("cd", 0)
        self.per_sample, self.copy = c.get("per_sample", False), c.get("copy", False)
        mo, mi = ref["mo"].cuda(), ref["mi"].cuda()
        if not self.per_sample:
            mo, mi = mo[0], mi[0]
        if self.copy:
            mi = mo
        self.plan = plan = ops.MeshPlan("euclid", mo, mi, c["loc"], self.copy)
        assert plan.nbr_idx is not None, "the case needs candidate lists"
        plan.ensure_reverse_lists()
        assert plan.rank_w == ref["w"]
        cnt, cap = plan.nbr_cnt.cpu(), plan.nbr_cap
        print(f"  cap {cap}, candidates {int(cnt.min())}..{int(cnt.max())}, kept {int(ref['kept'].min())}..{int(ref['kept'].max())}")
        if c.get("dup"):
            assert bool((cnt > cap).any()) == bool(c.get("overflow")) and bool((cnt <= cap).any())
        else:
            assert bool((cnt <= cap).all())
        if c.get("all_kept"):
            assert bool((ref["kept"] == cnt.view(ref["kept"].shape)).any()), "no row keeps all of its candidates"
        if c.get("shuffle"):                          # the chunked walks: unions beyond 64 keys per 16-row tile, 192 per 256-row block
            idx = plan.nbr_idx.cpu().view(plan.mesh_batch, plan.n_out, cap)[0]
            live = torch.arange(cap)[None, :] < cnt.view(plan.mesh_batch, plan.n_out)[0][:, None]
            union = lambda r0, n: int(torch.unique(idx[r0:r0 + n][live[r0:r0 + n]]).numel())
            tile, block = max(union(r0, 16) for r0 in range(0, plan.n_out, 16)), max(union(r0, 256) for r0 in range(0, plan.n_out, 256))
            print(f"  largest union: {tile} keys per tile, {block} per 256-row block")
            assert tile > 64 and block > 192
        self.complete = 0 if c.get("overflow") else 1
        if "cap" in c:
            assert cap == c["cap"]
        self.col0 = c.get("col0", self.dim if self.copy else 0)
        self.width = self.col0 + self.H * self.dim
        pad, gap, off = c.get("pad", 4), c.get("gap", 4), c.get("off", 0)
        self.V = Buf(self.b, plan.n_in, self.dim - self.cd, c.get("vpad", pad), gap, c.get("voff", off), data=ref["vals"])
        self.head = Buf(1, 1, self.H, data=ref["cvec"])
        self.mb = plan.mesh_batch
        self.tol = TOL[bool(c.get("out16") or c.get("dout16"))]

    # -- argument groups ------------------------------------------------------------------------------------------------
    def _mesh(self):
        p = self.plan
        return (p.mesh_out.data_ptr(), p.mesh_in.data_ptr(), p.mesh_batch, p.n_out, p.n_in, p.sdim, p.metric_id, p.period)

    def _values(self):
        return (self.V.ptr, self.b, self.dim, self.V.ld, self.V.bs)

    def _lists(self):
        p = self.plan
        return (p.nbr_idx.data_ptr(), p.nbr_cnt.data_ptr(), p.nbr_cap)

    def expect(self, **kw):
        """The record from the case's literals: rows=(NH, CR, gy), cols=(CR, gy), pair=(NH, CRR, CRC), union=(NH, EPL, per)."""
        e = {k: v for k, v in kw.items() if k in KINDS and v}
        if "rows" in kw:
            nh, cr, gy = kw["rows"]
            e.update(last_rows=nh * 100 + cr, last_grid_y=gy)
        if "cols" in kw:
            cr, gy = kw["cols"]
            e.update(last_cols=cr, last_grid_y=gy)
        if "pair" in kw:
            nh, crr, crc = kw["pair"]
            e.update(last_pair=nh * 10000 + crr * 100 + crc)
        if "union" in kw:
            nh, epl, per = kw["union"]
            e.update(last_union=nh * 100 + epl)
            if per:
                e.update(last_union_per=per)
        return e

    # -- pit_posatt_fwd_job -----------------------------------------------------------------------------------------------
    def forward(self, expect, mode=FP32, rc_want=0, head=None, is_scale=1, numeric=True, job=None):
        c, p, L = self.c, self.plan, _lib_()
        out16 = bool(mode & OUT16)
        out = Buf(self.b, p.n_out, self.width, c.get("opad", c.get("pad", 4)), c.get("gap", 4), c.get("ooff", c.get("off", 0)), bf16=out16)
        rowstat = Buf(1, self.mb * self.H * p.n_out, 4)
        scale_out = Buf(1, 1, self.H)
        head = self.head if head is None else head
        counts()
        rc = L.lib().pit_posatt_fwd_job(*self._mesh(), *self._values(), head.ptr, self.H, is_scale,
                                        p.stats.data_ptr(), p.rank_w, 1, 1 if self.copy else 0,
                                        out.ptr, out.ld, out.bs, self.col0, 1 if self.copy else 0, rowstat.ptr, scale_out.ptr,
                                        *self._lists(), self.cd, mode, L.stream_ptr(), job)
        torch.cuda.synchronize()
        got = counts()
        print(f"  forward: rc {rc}, record {got}")
        assert rc == rc_want
        assert got == expect
        if rc:
            assert out.unwritten() and rowstat.unwritten() and scale_out.unwritten()
            return None
        assert self.V.untouched() and head.untouched() and rowstat.untouched() and scale_out.untouched()
        r64 = self.ref["r64"]
        o, rs = out.cpu(), rowstat.cpu().view(self.mb, self.H, p.n_out, 4)
        assert bool(torch.isfinite(rs).all())
        assert out.untouched()
        if self.copy:
            assert torch.equal(o[..., :self.dim], self.ref["vals"]), "copy_inputs: columns [0, dim)"
        elif self.col0:                               # columns below out_col0 belong to the caller: never written
            below = out.buf.as_strided(out.shape, out.strides, out.start)[..., :self.col0]
            assert bool((below == out.fill).all()), "wrote below out_col0"
        o = o[..., self.col0:]
        if not numeric:
            return scale_out
        assert torch.equal(rs[..., 0], self.ref["T"]) and torch.equal(rs[..., 1], self.ref["smin"]), "T / S_min not bit-equal"
        assert torch.equal(scale_out.cpu().view(-1), self.ref["cvec"])
        compare("out", o, r64["out"], self.tol["fwd"])
        flat = lambda t: t.reshape(1, -1, 1)
        compare("1/L", flat(rs[..., 2]), flat(r64["invl"]), TOL[False]["fwd"], 1, 1)
        compare("mbar", flat(rs[..., 3]), flat(r64["mbar"]), TOL[False]["fwd"], 1, 1)
        return scale_out

    # -- pit_posatt_bwd ---------------------------------------------------------------------------------------------------
    def backward(self, expect, want_dv, want_dc, mode=FP32, rc_want=0, rev=True, complete=None, dense_dv=False, rider=None, **over):
        """d(values) and / or d(c) from the reference's rowstat (fp32 roundings of the fp64 1/L and mbar, the exact T and S_min)."""
        c, p, L, ref = self.c, self.plan, _lib_(), self.ref
        d16 = bool(mode & DOUT16)
        pad, gap, off = c.get("pad", 4), c.get("gap", 4), c.get("off", 0)
        dout = Buf(self.b, p.n_out, self.width, over.get("dpad", c.get("dpad", pad)), gap, over.get("doff", c.get("doff", off)), bf16=d16,
                   data=ref["dout"])
        rsd = torch.stack((ref["T"], ref["smin"], ref["r64"]["invl"].float(), ref["r64"]["mbar"].float()), -1)
        rowstat = Buf(1, self.mb * self.H * p.n_out, 4, data=rsd)
        dvb = Buf(self.b, p.n_in, self.dim - self.cd, 0 if dense_dv else over.get("dvpad", 4), 0 if dense_dv else gap) if want_dv else None
        dhead = Buf(1, 1, self.H) if want_dc else None
        work = torch.zeros(self.H * 1024, dtype=torch.float64, device="cuda")
        counts()
        rc = L.lib().pit_posatt_bwd(*self._mesh(), *self._values(), self.head.ptr, self.H, 1, None, rowstat.ptr, 1,
                                    dout.ptr, dout.ld, dout.bs, over.get("col0", self.col0),
                                    dvb.ptr if dvb else None, dvb.ld if dvb else 0, dvb.bs if dvb else 0, 1 if self.copy else 0,
                                    dhead.ptr if dhead else None, 0, work.data_ptr(), *self._lists(),
                                    self.complete if complete is None else complete,
                                    p.rev_ptr.data_ptr() if rev else None, p.rev_row.data_ptr() if rev else None, rider,
                                    self.cd, mode, L.stream_ptr())
        torch.cuda.synchronize()
        got = counts()
        print(f"  backward: rc {rc}, record {got}")
        assert rc == rc_want
        assert got == expect
        assert dout.untouched() and rowstat.untouched() and self.V.untouched() and self.head.untouched()
        assert float(work.abs().max()) == 0.0, "the fp64 d(scale) accumulators are not left zero"
        if rc:
            assert (dvb is None or dvb.unwritten()) and (dhead is None or dhead.unwritten())
            return
        r64 = ref["r64"]
        if dvb is not None:
            assert dvb.untouched()
            compare("d(values)", dvb.cpu(), r64["dv"], self.tol["dv"])
        if dhead is not None:
            assert dhead.untouched()
            compare("d(c)", dhead.cpu(), r64["dc"].reshape(1, 1, -1), self.tol["dc"], 1, 1)


GEOMETRY = ("n_out", "n_in", "batch", "dim", "heads", "sdim", "per_sample", "cd", "loc", "seed", "copy", "cloud", "shuffle", "dup", "dup_at",
            "cmul", "col0", "dout16")


def _case(id_, n_out, n_in, batch, dim, heads, loc=0.05, **kw):
    return pytest.param(dict(n_out=n_out, n_in=n_in, batch=batch, dim=dim, heads=heads, loc=loc, **kw), id=id_)


# --------------------------------------------------------------------------- the list kernels by (NH, CR)
# rows = (NH, CR, grid.y) of posatt_sparse_rows, cols = (CR, grid.y) of posatt_sparse_cols.  Shared meshes: ncols = batch * dim.
LIST = [
    _case("list-nh1-cr1-9x40", 9, 200, 2, 20, 1, rows=(1, 1, 1), cols=(1, 1)),
    _case("list-nh2-cr2-1025x130", 1025, 1100, 2, 65, 2, rows=(2, 2, 2), cols=(2, 2), col0=3),
    _case("list-nh2-cr2-2049x70", 2049, 300, 2, 35, 2, rows=(2, 2, 1), cols=(1, 2)),
    _case("list-nh1-cr2-gz3-343x130", 343, 300, 2, 65, 3, rows=(1, 2, 2), cols=(1, 3)),
    _case("list-nh1-cr4-2049x130", 2049, 2100, 2, 65, 1, loc=0.005, rows=(1, 4, 1), cols=(4, 1)),
    _case("list-nh2-cr4-1025x260", 1025, 1100, 4, 65, 2, rows=(2, 4, 2), cols=(4, 2)),
    _case("list-nh1-cr8-2049x260", 2049, 300, 2, 130, 1, rows=(1, 8, 1), cols=(1, 5)),
    _case("list-nh2-cr8-2049x260", 2049, 2049, 2, 130, 2, rows=(2, 8, 1), cols=(8, 1)),
    _case("list-nh2-cr8-1025x520", 1025, 700, 4, 130, 2, rows=(2, 8, 2), cols=(4, 3)),
    _case("list-nh2-cr8-gz2-513x520", 513, 450, 8, 65, 4, rows=(2, 8, 2), cols=(2, 5)),
    _case("list-per-sample-nh2-cr2-5x205x130", 205, 220, 5, 130, 2, rows=(2, 2, 2), cols=(2, 2), per_sample=True, cloud=True),
]


@pytest.mark.parametrize("c", LIST)
def test_list_kernels_by_instance(c):
    """Forward, d(scale) alone and d(values) alone of one (NH, CR) instance of the candidate-list kernels."""
    r = Run(c)
    r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]))
    r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, rows=c["rows"]), False, True)
    r.backward(r.expect(list_cols=1, cols=c["cols"]), True, False)


# --------------------------------------------------------------------------- the XCD-remapped twins
X = [
    _case("x-cr1-gy16-9x1000", 9, 200, 8, 125, 1, rows=(1, 1, 16), cols=(1, 16), x=True),
    _case("x-cr1-gy17-nh2-9x1030", 9, 200, 10, 103, 2, rows=(2, 1, 17), cols=(1, 17), x=True),
    _case("x-cr8-gy16-129x7690", 129, 200, 10, 769, 1, rows=(1, 8, 16), cols=(8, 16), x=True),
    _case("x-cr8-gy17-nh2-129x8200", 129, 200, 8, 1025, 2, rows=(2, 8, 17), cols=(8, 17), x=True),
    _case("x-cr8-gy23-130x11300", 130, 200, 10, 1130, 1, rows=(1, 8, 23), cols=(8, 23), x=True),
    _case("x-under-gy15-9x960", 9, 200, 8, 120, 1, rows=(1, 1, 15), cols=(1, 15), x=False),
]


@pytest.mark.parametrize("c", X)
def test_xcd_remapped_kernels(c):
    """posatt_sparse_rows_x (both modes) and posatt_sparse_cols_x from grid.y = 16 on, with grid.y % 8 = 0, 1 and 7; one column
    block fewer keeps the plain grids."""
    r = Run(c)
    if c["x"]:
        r.forward(r.expect(list_rows_x=1, rows=c["rows"]))
        r.backward(r.expect(list_rows_x=1, dhead_finish=1, rows=c["rows"]), False, True)
        r.backward(r.expect(list_cols_x=1, cols=c["cols"]), True, False)
    else:
        r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]))
        r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, rows=c["rows"]), False, True)
        r.backward(r.expect(list_cols=1, cols=c["cols"]), True, False)


# --------------------------------------------------------------------------- the merged backward
PAIR = [
    _case("pair-1-1", 9, 200, 2, 20, 1, pair=(1, 1, 1)),
    _case("pair-2-2", 1025, 1100, 2, 65, 2, pair=(2, 2, 2)),
    _case("pair-2-1", 1025, 300, 2, 65, 2, pair=(2, 2, 1)),
    _case("pair-4-4", 2049, 2100, 2, 65, 1, loc=0.005, pair=(1, 4, 4)),
    _case("pair-4-1", 1025, 300, 4, 65, 1, pair=(1, 4, 1)),
    _case("pair-8-8", 2049, 2049, 2, 130, 2, pair=(2, 8, 8)),
    _case("pair-8-1", 1025, 200, 4, 130, 2, pair=(2, 8, 1)),
]


@pytest.mark.parametrize("c", PAIR)
def test_merged_backward_by_instance(c):
    """d(scale) and d(values) in one launch: posatt_sparse_bwd_kernel<NH, CRR, CRC>."""
    r = Run(c)
    r.backward(r.expect(list_pair=1, dhead_finish=1, pair=c["pair"]), True, True)


def test_merged_backward_declined_above_16384_workgroups():
    """64 samples x 513 rows and 520 keys at one column per lane: 8208 + 8320 workgroups - the two launches run separately."""
    c = dict(n_out=513, n_in=520, batch=64, dim=40, heads=2, loc=0.0202, per_sample=True, cloud=True, seed=3)
    r = Run(c)
    r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, list_cols=1, rows=(2, 1, 1), cols=(1, 1)), True, True)


D16 = [
    _case("pair-d16-crr2", 1025, 300, 2, 66, 2, pair=(2, 2, 2), cols=(2, 2), dout16=True),
    _case("pair-d16-crr4", 1025, 300, 4, 66, 1, pair=(1, 4, 4), cols=(2, 3), dout16=True),
    _case("pair-d16-crr8", 1025, 200, 4, 130, 2, pair=(2, 8, 8), cols=(2, 5), dout16=True),
]
COLS16 = [      # d(values) alone: posatt_sparse_cols<4 | 8, true>, and the remapped posatt_sparse_cols_x<8, true> (grid.y = 16)
    _case("cols-d16-cr4", 45, 1100, 4, 66, 1, loc=0.0105, cols=(4, 2), dout16=True, x=False),
    _case("cols-d16-cr8", 45, 2100, 4, 66, 1, loc=0.005, cols=(8, 1), dout16=True, x=False),
    _case("cols-d16-cr8-x-gy16", 129, 200, 10, 770, 1, cols=(8, 16), dout16=True, x=True),
]


@pytest.mark.parametrize("c", D16)
def test_merged_backward_bf16_dout(c):
    """PIT_IO_DOUT_BF16: posatt_sparse_bwd_kernel<NH, CRR, CRR, true> (column pairs), then d(values) alone on posatt_sparse_cols<2, true>."""
    r = Run(c)
    r.backward(r.expect(list_pair_d16=1, dhead_finish=1, pair=c["pair"]), True, True, mode=BF16 | DOUT16)
    r.backward(r.expect(list_cols_d16=1, cols=c["cols"]), True, False, mode=BF16 | DOUT16)


@pytest.mark.parametrize("c", COLS16)
def test_dvalues_alone_bf16_dout(c):
    """posatt_sparse_cols<4, true>, <8, true> and the remapped posatt_sparse_cols_x<8, true> (it bumps both list_cols_d16 and
    list_cols_x)."""
    r = Run(c)
    r.backward(r.expect(list_cols_d16=1, list_cols_x=1 if c["x"] else 0, cols=c["cols"]), True, False, mode=BF16 | DOUT16)


def test_bf16_dout_below_two_columns_per_lane_and_refusals():
    """crr < 2: the pair is refused, d(values) runs posatt_sparse_cols<2, true> (max(2, cr)); odd dim / out_col0 / ld_dout and a d_out
    pointer two bytes off the 4-byte grid return PIT_ERR_UNSUPPORTED and write nothing."""
    c = dict(n_out=9, n_in=200, batch=2, dim=20, heads=1, loc=0.05, dout16=True, pad=4)
    r = Run(c)
    r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, list_cols_d16=1, rows=(1, 1, 1), cols=(2, 1)), True, True, mode=BF16 | DOUT16)
    r.backward({}, True, True, mode=BF16 | DOUT16, rc_want=UNSUPPORTED, dpad=5)              # odd ld_dout
    r.backward({}, True, True, mode=BF16 | DOUT16, rc_want=UNSUPPORTED, doff=1)              # d_out two bytes off
    r2 = Run(dict(c, col0=3, pad=5))
    r2.backward({}, True, True, mode=BF16 | DOUT16, rc_want=UNSUPPORTED)                     # odd out_col0
    r3 = Run(dict(c, dim=21, pad=5))
    r3.backward({}, True, True, mode=BF16 | DOUT16, rc_want=UNSUPPORTED)                     # odd dim


# --------------------------------------------------------------------------- list lengths, gather-group tails
TAIL = [
    # kept counts k + 1 = 11 (not a multiple of G = 8, 4 or 2) at CR 1, 4 and 8
    _case("tail-kept11-cr1", 9, 200, 2, 20, 1, loc=0.0525, rows=(1, 1, 1), cols=(1, 1), kept=11),
    _case("tail-kept11-cr4", 2049, 2100, 2, 65, 1, loc=0.00497, rows=(1, 4, 1), cols=(4, 1), kept=11),
    _case("tail-kept11-cr8", 2049, 2049, 2, 130, 2, loc=0.0051, rows=(2, 8, 1), cols=(8, 1), kept=11),
    # lists longer than one 64-lane pass (rank_k + 2 = 69 of 400 keys)
    _case("tail-long-lists", 37, 400, 2, 20, 2, loc=0.17, rows=(2, 1, 1), cols=(1, 1), kept=68, cap=96),
    # rank_k = 0: every row keeps exactly its nearest key
    _case("tail-one-key", 37, 200, 2, 20, 1, loc=0.004, rows=(1, 1, 1), cols=(1, 1), kept=1),
    # 20 duplicated keys under a capacity of 32: the rows sitting on them keep every candidate they have (20), rows whose k-th
    # neighbour is one of the 20 keep those and the nearer ones (up to 27)
    _case("tail-keeps-all-candidates", 37, 200, 2, 20, 1, rows=(1, 1, 1), cols=(1, 1), dup=(20, 3), dup_at=5, kept=27, all_kept=True),
]


@pytest.mark.parametrize("c", TAIL)
def test_list_lengths_and_group_tails(c):
    r = Run(c)
    assert int(r.ref["kept"].max()) == c["kept"]
    r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]))
    r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, rows=c["rows"]), False, True)
    r.backward(r.expect(list_cols=1, cols=c["cols"]), True, False)


# --------------------------------------------------------------------------- overflowed rows
OVER = [
    _case("over-shared", 41, 240, 2, 20, 2, cloud=True, dup=(60, 10), dup_at=7, overflow=True, rows=(2, 1, 1), cols=(1, 1)),
    _case("over-per-sample", 41, 240, 2, 20, 2, cloud=True, dup=(60, 10), dup_at=7, overflow=True, per_sample=True, rows=(2, 1, 1), cols=(1, 1)),
    _case("over-coord2", 41, 240, 2, 20, 1, cloud=True, dup=(60, 10), dup_at=7, overflow=True, cd=2, rows=(1, 1, 1), cols=(1, 1)),
]


@pytest.mark.parametrize("c", OVER)
def test_overflowed_rows_next_to_listed_rows(c):
    """60 duplicated keys overflow the 32-slot lists of the 10 rows sitting on them: those rows scan every key in the forward and in
    d(scale); d(values) takes the listed rows from the transposed lists and the overflowed ones from posatt_sparse_overflow_cols."""
    r = Run(c)
    r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]))
    r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, rows=c["rows"]), False, True)
    r.backward(r.expect(list_cols=1, list_overflow=1, cols=c["cols"]), True, False)
    r.backward(r.expect(list_pair=1, list_overflow=1, dhead_finish=1, pair=(c["rows"][0], 1, 1)), True, True)


def test_complete_plan_skips_the_overflow_pass():
    c = dict(n_out=41, n_in=240, batch=2, dim=20, heads=2, loc=0.05, cloud=True)
    r = Run(c)
    r.backward(r.expect(list_cols=1, cols=(1, 1)), True, False, complete=1)
    r.backward(r.expect(list_cols=1, list_overflow=1, cols=(1, 1)), True, False, complete=0)


def test_dvalues_without_transposed_lists_runs_the_dense_kernel():
    """d(values) of a list layer whose plan carries no transposed lists (and no union form asked for) is launch_cols' business: the
    one coarse `dense` kind, no list kind."""
    r = Run(dict(n_out=41, n_in=240, batch=2, dim=20, heads=2, loc=0.05, cloud=True))
    r.backward(r.expect(dense=1), True, False, rev=False)


# --------------------------------------------------------------------------- coordinate channels, the concat form
COORD = [
    _case("coord1-cr1", 9, 200, 2, 21, 1, cd=1, sdim=1, rows=(1, 1, 1), cols=(1, 1)),
    _case("coord2-cr1", 9, 200, 2, 21, 1, cd=2, rows=(1, 1, 1), cols=(1, 1)),
    _case("coord2-cr8", 2049, 2049, 2, 131, 2, cd=2, rows=(2, 8, 1), cols=(8, 1)),
    _case("coord1-cr8-sdim3", 1025, 1100, 4, 130, 2, loc=0.0105, cd=1, sdim=3, rows=(2, 8, 2), cols=(8, 2)),
]


@pytest.mark.parametrize("c", COORD)
def test_coordinate_channels(c):
    """coord_dims > 0: value channels [0, coord_dims) are the key's coordinates, read from mesh_in; d(values) has the others."""
    r = Run(c)
    r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]))
    r.backward(r.expect(list_cols=1, cols=c["cols"]), True, False)


def test_concat_form_and_its_refusals():
    """copy_inputs (masked self attention into a concat buffer, out_col0 = dim, add_residual in the backward); coord_dims or a bf16
    out together with copy_inputs are refused."""
    c = dict(n_out=203, n_in=203, batch=2, dim=20, heads=2, loc=0.05, copy=True)
    r = Run(c)
    r.forward(r.expect(list_rows_fwd=1, rows=(2, 1, 1)))
    r.backward(r.expect(list_pair=1, dhead_finish=1, pair=(2, 1, 1)), True, True)
    r.backward(r.expect(list_cols=1, cols=(1, 1)), True, False)
    r.forward({}, mode=BF16 | OUT16, rc_want=UNSUPPORTED)
    Run(dict(c, cd=1)).forward({}, rc_want=UNSUPPORTED)


def test_bf16_stored_out():
    """PIT_IO_OUT_BF16 on the list kernels at CR 1 and CR 8."""
    for c in (dict(n_out=9, n_in=200, batch=2, dim=20, heads=1, loc=0.05, out16=True, rows=(1, 1, 1)),
              dict(n_out=2049, n_in=2049, batch=2, dim=130, heads=2, loc=0.05, out16=True, rows=(2, 8, 1))):
        r = Run(c)
        r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]), mode=BF16 | OUT16)


# --------------------------------------------------------------------------- union tiles
# union = (NH, EPL, per).  cap <= 32: EPL 8 (loc 0.05 of 200 keys: cap 32); cap 48: EPL 16 (loc 0.1 of 256 keys).
UNI = [
    _case("union-one-tile-nh1-epl8", 16, 200, 2, 24, 1, union=(1, 8, 1), cols=(1, 1)),
    _case("union-13-of-16-nh2-epl16", 77, 256, 3, 40, 2, loc=0.1, union=(2, 16, 1), cols=(1, 2), cap=48),
    _case("union-nh1-epl16", 77, 256, 2, 24, 1, loc=0.1, union=(1, 16, 1), cols=(1, 1), cap=48),
    _case("union-one-live-wave-nh2-epl8", 69, 200, 2, 72, 2, union=(2, 8, 1), cols=(1, 3)),
    _case("union-last-bitmap-word-4096", 45, 4096, 1, 24, 1, loc=0.002, union=(1, 8, 1), cols=(1, 1)),
    _case("union-shuffled-rows", 523, 700, 2, 24, 2, loc=0.02, shuffle=True, union=(2, 8, 1), cols=(1, 1)),
    _case("union-overflowed-row", 45, 240, 2, 24, 2, cloud=True, dup=(60, 1), dup_at=21, overflow=True, union=(2, 8, 1), cols=(1, 1)),
    _case("union-per-sample", 45, 200, 3, 40, 2, per_sample=True, union=(2, 8, 1), cols=(1, 1)),
    _case("union-per2-ncb3-16397x320", 16397, 256, 4, 80, 1, loc=0.03, union=(1, 8, 2), cols=(1, 5)),
    _case("union-per2-ncb2-32770x256", 32770, 256, 2, 128, 1, loc=0.03, union=(1, 8, 2), cols=(1, 4)),
    _case("union-per8-ncb5-33000x520", 33000, 256, 5, 104, 1, loc=0.03, union=(1, 8, 8), cols=(1, 9)),
]


@pytest.mark.parametrize("c", UNI)
def test_union_tiles(c):
    """PIT_ATT_UNION: forward and d(scale) on posatt_union_kernel; d(values) from the transposed lists when they are given, from
    zero_f32_kernel + posatt_union_dv_kernel (fp32 atomics, a dense d_values) when they are not."""
    r = Run(c)
    nh, epl, per = c["union"]
    r.forward(r.expect(union_fwd=1, union=c["union"]), mode=UNION)
    r.backward(r.expect(union_dscale=1, dhead_finish=1, union=c["union"]), False, True, mode=UNION)
    r.backward(r.expect(union_zero=1, union_dv=1, union=(nh, epl, 0)), True, False, mode=UNION, rev=False, dense_dv=True)
    over = dict(list_overflow=1) if c.get("overflow") else {}
    r.backward(r.expect(list_cols=1, cols=c["cols"], **over), True, False, mode=UNION, dense_dv=True)


def test_union_tiles_bf16_storage():
    """PIT_IO_OUT_BF16 / PIT_IO_DOUT_BF16 with the union form (16-byte pieces of 8 elements)."""
    c = dict(n_out=77, n_in=200, batch=2, dim=24, heads=2, loc=0.05, out16=True, dout16=True, pad=8, gap=0)
    r = Run(c)
    r.forward(r.expect(union_fwd=1, union=(2, 8, 1)), mode=BF16 | OUT16 | UNION)
    r.backward(r.expect(union_dscale=1, dhead_finish=1, union=(2, 8, 1)), False, True, mode=BF16 | DOUT16 | UNION)
    r.backward(r.expect(union_zero=1, union_dv=1, union=(2, 8, 0)), True, False, mode=BF16 | DOUT16 | UNION, rev=False, dense_dv=True)


DECL = [
    _case("decl-dim-not-8", 45, 200, 2, 20, 2, rows=(2, 1, 1)),
    _case("decl-ld-values-not-4", 45, 200, 2, 24, 2, vpad=1, rows=(2, 1, 1)),
    _case("decl-out-col0-not-4", 45, 200, 2, 24, 2, col0=2, opad=2, dpad=2, rows=(2, 1, 1)),      # (ld_out = ld_dout = 52: only col0 declines)
    _case("decl-values-4-bytes-off", 45, 200, 2, 24, 2, voff=1, rows=(2, 1, 1)),
    _case("decl-cap-over-64", 45, 400, 2, 24, 2, loc=0.15, cap=80, rows=(2, 1, 1)),
    _case("decl-15-rows", 15, 200, 2, 24, 2, rows=(2, 1, 1)),
    _case("decl-4097-keys", 45, 4097, 1, 24, 2, loc=0.002, rows=(2, 1, 1)),
    _case("decl-three-heads", 45, 200, 2, 24, 3, rows=(1, 1, 1)),
    _case("decl-coord-dims", 45, 200, 2, 24, 2, cd=1, vpad=1, rows=(2, 1, 1)),                    # (23 value channels, ld_values = 24)
]


@pytest.mark.parametrize("c", DECL)
def test_union_form_declined(c):
    """PIT_ATT_UNION on shapes the union tiles do not take: the list kernels run and the result is still right."""
    r = Run(c)
    r.forward(r.expect(list_rows_fwd=1, rows=c["rows"]), mode=UNION)
    r.backward(r.expect(list_rows_dscale=1, dhead_finish=1, rows=c["rows"]), False, True, mode=UNION)


def test_union_backward_declined_for_residual_and_strided_dvalues():
    """add_residual (the concat form) and a d_values with padded rows keep the whole backward on the list kernels - the merged
    launch; the same call with a dense d_values takes d(scale) from the tiles."""
    r = Run(dict(n_out=203, n_in=203, batch=2, dim=24, heads=2, loc=0.05, copy=True))
    r.backward(r.expect(list_pair=1, dhead_finish=1, pair=(2, 1, 1)), True, True, mode=UNION, dense_dv=True)
    r = Run(dict(n_out=45, n_in=200, batch=2, dim=24, heads=2, loc=0.05))
    r.backward(r.expect(list_pair=1, dhead_finish=1, pair=(2, 1, 1)), True, True, mode=UNION)            # (ld_dvalues = dim + 4)
    r.backward(r.expect(union_dscale=1, dhead_finish=1, list_cols=1, union=(2, 8, 1), cols=(1, 1)), True, True, mode=UNION, dense_dv=True)


# --------------------------------------------------------------------------- 4..8 coordinates
def test_meshes_of_5_coordinates():
    """posatt_sparse_rows8 / _cols8 / _overflow_cols8: no pair launch, no remap, whatever the width."""
    c = dict(n_out=41, n_in=240, batch=2, dim=20, heads=2, loc=0.05, sdim=5, cloud=True, dup=(60, 10), dup_at=7, overflow=True)
    r = Run(c)
    r.forward(r.expect(list_rows8=1))
    r.backward(r.expect(list_rows8=1, dhead_finish=1, list_cols8=1, list_overflow8=1), True, True)
    r = Run(dict(n_out=41, n_in=240, batch=2, dim=20, heads=2, loc=0.05, sdim=5, cloud=True, dout16=True))
    r.backward(r.expect(list_cols8=1), True, False, mode=BF16 | DOUT16)                                 # posatt_sparse_cols8<2, true>
    wide = dict(n_out=9, n_in=200, batch=8, dim=125, heads=1, loc=0.05, sdim=4, cloud=True)            # grid.y = 16: still no remap
    r = Run(wide)
    r.forward(r.expect(list_rows8=1))
    r.backward(r.expect(list_rows8=1, dhead_finish=1, list_cols8=1), True, True)


# --------------------------------------------------------------------------- launches that carry a rider
class Rider:
    """A small postponed pit_mlp_bwd_params job (random operands: its results are tests/test_gpu_riders.py's business)."""

    def __init__(self):
        import ctypes
        rows, n0, n1, n2 = 256, 24, 16, 8
        self.keep = [torch.randn(s, device="cuda") for s in ((rows, n0), (rows, n1), (rows, n2), (rows * (n1 + n2),))]
        self.grads = [torch.zeros(s, device="cuda") for s in ((n1, n0), (n1,), (n2, n1), (n2,))]
        x, h, dy, scratch = self.keep
        self.job = _lib_().MlpParamsJob(x.data_ptr(), n0, rows, n0, n1, n2, h.data_ptr(), 1, dy.data_ptr(), n2,
                                        *[g.data_ptr() for g in self.grads], 1, scratch.data_ptr(), 0)
        self.ptr = ctypes.cast(ctypes.pointer(self.job), ctypes.c_void_p)

    def delivered(self):
        torch.cuda.synchronize()
        return all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in self.grads)


class Weights:
    """A pit_block_weights job on a 64-point latent mesh, one layer."""

    def __init__(self, n_head=2):
        import ctypes
        L = 64
        self.mesh = lattice(L, 2, 77).cuda()
        self.head = torch.tensor([1.5, 2.5][:n_head], device="cuda")
        self.hp = (ctypes.c_void_p * 1)(self.head.data_ptr())
        self.e, self.inv = torch.zeros(1, n_head, L, L, device="cuda"), torch.zeros(1, n_head, L, device="cuda")
        self.rowstat, self.scale = torch.zeros(1, n_head, L, 4, device="cuda"), torch.zeros(1, n_head, device="cuda")
        self.job = _lib_().BlockWeightsJob(self.mesh.data_ptr(), L, 2, 0, 0.0, 1, ctypes.cast(self.hp, ctypes.c_void_p), 1, n_head,
                                           self.e.data_ptr(), None, self.inv.data_ptr(), self.rowstat.data_ptr(), self.scale.data_ptr())
        self.ptr = ctypes.cast(ctypes.pointer(self.job), ctypes.c_void_p)

    def delivered(self):
        torch.cuda.synchronize()
        return torch.equal(self.scale.cpu().view(-1), self.head.cpu()) and float(self.inv.min()) > 0


def test_rider_carried_by_the_list_launches():
    """A postponed weight-gradient job rides in posatt_sparse_rows_dw (d(scale) alone) and posatt_sparse_bwd_dw_kernel (the pair);
    the attention results are the plain launches'."""
    r = Run(dict(n_out=9, n_in=200, batch=2, dim=20, heads=1, loc=0.05))
    rd = Rider()
    r.backward(r.expect(list_rows_dw=1, dhead_finish=1, rows=(1, 1, 1)), False, True, rider=rd.ptr)
    assert rd.delivered()
    rd = Rider()
    r.backward(r.expect(list_pair_dw=1, dhead_finish=1, pair=(1, 1, 1)), True, True, rider=rd.ptr)
    assert rd.delivered()


@pytest.mark.parametrize("n_out,carried,seed", [(65536, True, 3), (65540, False, 2)])       # (seeds: the 4-ulp condition)
def test_rider_size_limit_of_the_dscale_launch(n_out, carried, seed):
    """16384 attention workgroups carry the job, 16385 leave it to a launch of its own."""
    r = Run(dict(n_out=n_out, n_in=200, batch=2, dim=20, heads=1, loc=0.0525, seed=seed))
    rd = Rider()
    kind = dict(list_rows_dw=1) if carried else dict(list_rows_dscale=1)
    r.backward(r.expect(dhead_finish=1, rows=(1, 1, 1), **kind), False, True, rider=rd.ptr)
    assert rd.delivered()


@pytest.mark.parametrize("n_out,carried,seed", [(45, True, 2), (16384, True, 3), (16388, False, 2)])
def test_block_weights_job_in_the_forward(n_out, carried, seed):
    """pit_posatt_fwd_job: up to 4096 attention workgroups form the processor's block weights in the same launch
    (posatt_sparse_rows_w), 4097 leave them to pit_block_weights right after it."""
    r = Run(dict(n_out=n_out, n_in=200, batch=2, dim=20, heads=2, loc=0.0525, seed=seed))
    w = Weights()
    kind = dict(list_rows_w=1) if carried else dict(list_rows_fwd=1)
    r.forward(r.expect(rows=(2, 1, 1), **kind), job=w.ptr)
    assert w.delivered()


# --------------------------------------------------------------------------- the record itself
def test_record_is_per_thread_and_resets():
    import threading
    r = Run(dict(n_out=9, n_in=200, batch=2, dim=20, heads=1, loc=0.05))
    r.forward(r.expect(list_rows_fwd=1, rows=(1, 1, 1)))
    r.forward(r.expect(list_rows_fwd=1, rows=(1, 1, 1)))
    from position_induced_transformer_amd import ops
    L = _lib_()
    out, rowstat = Buf(2, 9, 20), Buf(1, 9, 4)
    call = lambda: L.lib().pit_posatt_fwd_job(*r._mesh(), *r._values(), r.head.ptr, 1, 1, r.plan.stats.data_ptr(), r.plan.rank_w, 1, 0,
                                              out.ptr, out.ld, out.bs, 0, 0, rowstat.ptr, None, *r._lists(), 0, 0, L.stream_ptr(), None)
    assert call() == 0 and call() == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.att_launch_counts(reset=True)))
    t.start()
    t.join()
    assert not any(seen[0]), "another thread sees this thread's launches"
    assert counts(reset=False) == dict(list_rows_fwd=2, last_rows=101, last_grid_y=1)          # ... and did not reset them
    assert counts() == dict(list_rows_fwd=2, last_rows=101, last_grid_y=1) and counts() == {}
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- the head as lmda
def _ulps(a, b):
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("c", [
    _case("lmda-list-small", 45, 200, 2, 24, 2, want=dict(list_rows_fwd=1, rows=(2, 1, 1)), mode=FP32),
    _case("lmda-list-8193-rows", 8193, 200, 2, 24, 2, loc=0.0525, want=dict(list_rows_fwd=1, head_scale=1, rows=(2, 1, 1)), mode=FP32),
    _case("lmda-union", 45, 200, 2, 24, 2, want=dict(union_fwd=1, head_scale=1, union=(2, 8, 1)), mode=UNION),
])
def test_head_handed_over_as_lmda(c):
    """head_is_scale = 0: scale_out within 24 ulp of the oracle's head_scale (tests/test_gpu_ops.py); pit_head_scale runs up front for
    the union form and above 8192 rows, inside the rows kernel otherwise."""
    r = Run(c)
    lmda = torch.tensor([0.3, -0.7])
    head = Buf(1, 1, 2, data=lmda)
    so = r.forward(r.expect(**c["want"]), mode=c["mode"], head=head, is_scale=0, numeric=False)
    assert _ulps(so.cpu().view(-1), orc.head_scale(lmda)) <= 24

