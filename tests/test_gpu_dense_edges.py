"""The DENSE (MFMA) position-attention kernels of csrc/pit_posatt.hip - posatt_rows_kernel / posatt_cols_kernel (the J-split kernels),
posatt_bwd_pair_kernel / _pair_wide_kernel / _pair_dw_kernel, posatt_rows_tiles / posatt_cols_tiles (the large regime, also on
precomputed weights) and posatt_rows_kernel8 / posatt_cols_kernel8 (4..8 coordinates) - one dispatch instance at a time, through the
raw C ABI: pit_posatt_fwd / pit_posatt_bwd with nbr_idx = nbr_cnt = NULL, pit_posatt_pre_fwd / _bwd.  The machinery (Buf, block_errs,
compare, lattice, _evaluate) is tests/test_gpu_att_edges.py's; the reference builder below adds what the dense path adds (unmasked
layers, NULL statistics, periodic metrics, strides, the bf16 emulation).

Every GPU case

* resets both launch records (pit_debug_dense_counts, pit_debug_att_counts), runs ONE entry and asserts the exact dense record -
  counters, the packed template arguments of the PIT_DENSE_LAST_* slots (include/pit_hip.h) and the grid - and that PIT_ATT_DENSE
  counts the launches made through launch_rows / launch_cols / launch_bwd_pair (the pre entries call the tiles launchers
  themselves: PIT_ATT_DENSE stays 0 there).  The instance is a literal of the case (`rows=(CT, waves, IL)`, `trows=(RT, TPWG)`,
  `grid=(x, y, z)`), never recomputed from choose_ct or the regime rules: a retuned rule fails the case;
* hands every tensor as a view inside a NaN-filled allocation (Buf: guard rows, ld > width, gap rows between samples; SBuf adds a
  sample stride that is no multiple of the row pitch): every word outside an output's view still holds the pattern afterwards, every
  payload element is finite, the fp64 d(scale) slots are zero again after a non-deferred backward;
* compares with fp64 on the CPU, the mask as oracle/pit_oracle.py defines it (fp32 distances, row_order_stats, fp32 m * c, fp32 lerp;
  T = +inf unmasked, S_min = 0 without statistics), per block of ONE MFMA tile in the kernels' column space (32 rows x 32 columns of a
  head's batch * dim columns; 32 keys x 32 columns for d(values)); 1/L and mbar per row, T and S_min bit for bit.  A backward takes
  the REFERENCE's rowstat (rounded to fp32) as its input;
* asserts the 4-ulp mask condition of tests/test_gpu_att_edges.py on the reference alone (the seeds are chosen for it).

Bounds per block.  fp32 math: forward, 1/L, mbar 2e-6, d(values) 1e-5, d(c) 1e-4 (tests/test_gpu_att_edges.py).  PIT_MATH_BF16: d(c)
keeps 1e-4 (the rows kernels run bf16 in the forward only: MODE 1 is exact fp32), 1/L and mbar keep 2e-6 (summed from the fp32
weights); out and d(values) max(2e-2 / 5e-2 of tests/test_gpu_bf16.py, 2 x the per-block distance between the fp64 reference and a
CPU emulation that rounds both operands to bf16 (RNE) and accumulates in fp64) - formed from the references alone.
Worst blocks measured on an MI355X over all cases: fp32 math - out 8.7e-7, 1/L 3.1e-7, mbar 4.4e-7, d(values)
9.0e-7, d(c) 5.7e-6; bf16 math - out 3.7e-3, d(values) 3.9e-3, d(c) 4.4e-7, 1/L 3.1e-7, mbar 4.4e-7; precomputed weights - out 6.5e-7 /
3.1e-3 (fp32 / bf16), d(values) 5.6e-8 / 3.2e-3, d(c) 1.2e-6.  The worst bf16 emulation distances are 3.7e-3 (out) and 3.9e-3
(d(values)): twice that stays under the floors, so no block's bound was widened.

Case ids -> kernel template instances (the with_int / with_bool ladders of launch_rows, launch_cols, launch_bwd_pair,
launch_rows_tiles, launch_cols_tiles, launch_rows8, launch_cols8):

* ``rows-ct{1,2,4}-w{1,2,4,8}[-masked]`` posatt_rows_kernel<CT, 0 | 1, M, BF, IL>: every (CT, waves) of the dispatch (4 waves at most
  with CT 4), unmasked and masked, each forward fp32, forward bf16 and d(scale);
* ``cols-ct{1,2,4}-w{1,2,4,8}[-masked]`` posatt_cols_kernel<CT, M, BF, IL>, fp32 and bf16;
* ``il-*`` the IL = true instances of all three (CT 4) next to their IL = false twins, one declining condition at a time;
* ``chunk-*`` KEY_CHUNK (2048 keys) and ROW_CHUNK (1024 rows) seams of rows, cols and pair;
* ``pair-*`` posatt_bwd_pair_kernel<M, BF>, posatt_bwd_pair_wide_kernel<2 | 4, M, BF, IL>, posatt_bwd_pair_dw_kernel<M, BF>
  (``pair-dw-rider``), the wide kernel with its rider (``pair-wide-rider``) and the three declines;
* ``tiles-r{RT}x{TPW}-*`` posatt_rows_tiles<RT, TPW, 0 | 1, M, BF, false>, ``tiles-cols-{8,16,32}`` posatt_cols_tiles<TPW, M, BF, false>,
  ``tiles-unforced-*`` the work threshold without the environment;
* ``pre-*`` posatt_rows_tiles<1 | 2 | 4, 1, 0 | 1, false, BF, true> and posatt_cols_tiles<1, false, BF, true>; ``pre-r1x2-*``,
  ``pre-r1x4-*``, ``pre-r2x2-*`` the rows instances <1, 2>, <1, 4>, <2, 2> and posatt_cols_tiles<2 | 4, false, BF, true>;
* ``wide-*`` posatt_rows_kernel8<MODE, M, BF>, posatt_cols_kernel8<M, BF>;
* ``metric-*`` the PER variant of the step (J-split and tiles); ``form-*`` call forms and refusals; ``slow-*`` PIT_NO_FAST_LOADS;
  ``dup-*`` duplicated keys (exact ties at the threshold).

Cannot reach (listed, not forced; each read from the launcher named):

* IL with CT != 4: `il = ct == 4 && interleave_ok(...)` in launch_rows / launch_cols / launch_bwd_pair, the ladders leave it out;
* BF with MODE 1: `bf = (MODE == 0) && a.bf16` in launch_rows, launch_rows_tiles and launch_rows8;
* PRE with MASKED: fill_pre leaves masked = 0, launch_rows_pre / launch_cols_pre are the only callers with pre = true;
* RT x TPW > 4 (posatt_rows_tiles<2, 4>, <4, 2>, <4, 4>): rows_tiles_regime clamps tpwg to 8 at rt = 4 and to 16 at rt = 2;
* posatt_bwd_pair_dw_kernel at one wave: launch_bwd_pair carries the rider at nwaves >= 2 only;
* the PIT_EXPERIMENTS switches (PIT_FORCE_CT, PIT_FORCE_WAVES, ...): compiled out of the production library.
"""
import ctypes
import functools
import threading

import pytest
import torch

import pit_oracle as orc
from test_gpu_att_edges import BF16, FP32, GUARD, UNSUPPORTED, Buf, Rider, _evaluate, block_errs, compare, lattice
from test_gpu_att_edges import counts as att_counts

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_SIZE = -1, -2
OUT16, DOUT16 = 0x800, 0x1000
HEAD_ACCUMULATE, HEAD_DEFER, HEAD_IS_SCALE = 1, 2, 4
SLOTS = 1024                                  # PIT_DSCALE_SLOTS
TOL = dict(fwd=2e-6, dv=1e-5, dc=1e-4)        # fp32 math, per block
TOL_BF = dict(fwd=2e-2, dv=5e-2)              # bf16 math: the floor of max(floor, 2 x emulation distance)
METRIC = dict(euclid=0, periodic1d=1, periodic2d=2)

DKINDS = ("rows_fwd", "rows_dscale", "cols", "pair", "pair_wide", "pair_dw", "tiles_rows_fwd", "tiles_rows_dscale", "tiles_cols",
          "rows8", "cols8", "last_rows", "last_cols", "last_pair", "last_tiles_rows", "last_tiles_cols", "grid_x", "grid_y",
          "grid_z")                           # PIT_DENSE_* in order
COUNTERS = DKINDS[:11]


def dense_counts(reset=True):
    from position_induced_transformer_amd import ops
    c = ops.dense_launch_counts(reset=reset)
    assert len(c) == len(DKINDS)
    return {k: v for k, v in zip(DKINDS, c) if v}


def _pack(ct, waves, il, masked, bf):
    return ct * 10000 + waves * 1000 + int(il) * 100 + int(masked) * 10 + int(bf)


def _tpack(rt, tpwg, masked, bf, pre):
    return rt * 100000 + tpwg * 1000 + int(masked) * 100 + int(bf) * 10 + int(pre)


def record(spec, masked, bf, rows_mode, pre=False):
    """The dense record a call must leave, from the case's literals.  `spec` keys: rows / cols / pair = (CT, waves, IL), rows8 / cols8 =
    waves, trows = (RT, TPWG), tcols = TPWG, grid = (x, y, z) of the LAST launch, pair_kind = the pair's counter when it carries a
    rider.  `bf`: bf16 math asked for (d(scale) instances are fp32 whatever it says)."""
    e = {}
    bf_rows = bf and rows_mode == "fwd"
    for k, v in spec.items():
        if k == "rows":
            e["rows_" + rows_mode], e["last_rows"] = 1, _pack(*v, masked, bf_rows)
        elif k == "rows8":
            e["rows8"], e["last_rows"] = 1, _pack(1, v, 0, masked, bf_rows)
        elif k == "trows":
            e["tiles_rows_" + rows_mode], e["last_tiles_rows"] = 1, _tpack(v[0], v[1], masked, bf_rows, pre)
        elif k == "cols":
            e["cols"], e["last_cols"] = 1, _pack(*v, masked, bf)
        elif k == "cols8":
            e["cols8"], e["last_cols"] = 1, _pack(1, v, 0, masked, bf)
        elif k == "tcols":
            e["tiles_cols"], e["last_tiles_cols"] = 1, _tpack(0, v, masked, bf, pre)
        elif k == "pair":
            e[spec.get("pair_kind", "pair" if v[0] == 1 else "pair_wide")], e["last_pair"] = 1, _pack(*v, masked, bf)
        elif k == "grid":
            e.update(grid_x=v[0], grid_y=v[1], grid_z=v[2])
        else:
            assert k == "pair_kind", k
    return e


class SBuf(Buf):
    """Buf with `skew` more elements between samples: a sample stride that is no multiple of the row pitch."""

    def __init__(self, b, rows, n, pad=0, gap=0, off=0, skew=0, data=None):
        self.shape, self.ld, self.fill = (b, rows, n), n + pad, 0x7FC0BEEF
        self.bs = (rows + gap) * self.ld + skew
        self.strides, self.start = (self.bs, self.ld, 1), GUARD * self.ld + off
        total = 2 * GUARD * self.ld + b * self.bs + off + 8
        self.buf = torch.full((total,), self.fill, dtype=torch.int32, device="cuda")
        self.t = self.buf.view(torch.float32).as_strided(self.shape, self.strides, self.start)
        if data is not None:
            self.t.copy_(data.reshape(self.shape))


def compare_bf(name, got, ref64, emu, floor):
    """bf16 math: every block within max(floor, 2 x the block's distance between the bf16 emulation and the fp64 reference)."""
    e, d = block_errs(got, ref64, 32, 32), block_errs(emu, ref64, 32, 32)
    print(f"  {name}: worst block {float(e.max()):.3e} (floor {floor:.0e}, worst emulation distance {float(d.max()):.3e})")
    assert bool(torch.isfinite(e).all()), f"{name}: NaN or inf in the payload"
    bad = e > torch.clamp(2.0 * d, min=floor)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} blocks over the bound, worst {float(e.max()):.3e}"


# --------------------------------------------------------------------------- references (once per geometry, never modified)
GEOMETRY = ("n_out", "n_in", "batch", "dim", "heads", "sdim", "per_sample", "loc", "seed", "self_attn", "metric", "dup", "cmul", "col0")


def _meshes(c, i):
    n_out, n_in, sdim, seed, metric = c["n_out"], c["n_in"], c.get("sdim", 2), c.get("seed", 1), c.get("metric", "euclid")
    g = torch.Generator().manual_seed(100 * seed + i)
    if metric == "periodic1d":              # a uniform periodic line; rows 0..2 sit at the wrap
        mi = (torch.arange(n_in, dtype=torch.float32) / n_in)[:, None].contiguous()
        mo = torch.rand(n_out, 1, generator=g)
        mo[0], mo[1], mo[2] = 0.0013, 0.9991, 0.9969
        return mo, mi
    if metric == "periodic2d":              # a square periodic grid; rows 0..2 sit at an edge or a corner
        res = int(round(n_in ** 0.5))
        assert res * res == n_in
        mi = orc.grid_mesh_2d(res, endpoint=False)
        mo = torch.rand(n_out, 2, generator=g)
        mo[0], mo[1], mo[2] = torch.tensor([0.0013, 0.0021]), torch.tensor([0.9991, 0.5]), torch.tensor([0.4, 0.9987])
        return mo, mi
    mi = lattice(n_in, sdim, 100 * seed + i)
    mo = mi if c.get("self_attn") else lattice(n_out, sdim, 100 * seed + 50 + i, jitter=0.35)
    dup, rows_dup = c.get("dup", (0, 0))
    if dup:                                 # duplicated keys and the rows sitting on them
        mi = mi.clone()
        mi[:dup] = mi[:1]
        mo = mi if c.get("self_attn") else mo.clone()
        mo[5:5 + rows_dup] = mi[:1]
    return mo.contiguous(), mi.contiguous()


@functools.lru_cache(maxsize=3)
def reference(key):
    """Inputs and fp64 references of one geometry (the hashable GEOMETRY items of a case)."""
    c = dict(key)
    n_out, n_in, b, dim, H = c["n_out"], c["n_in"], c["batch"], c["dim"], c["heads"]
    loc, seed, metric, self_attn = c.get("loc", 1.0), c.get("seed", 1), c.get("metric", "euclid"), c.get("self_attn", False)
    masked, mb = loc < 1.0, (b if c.get("per_sample") else 1)
    assert not self_attn or n_out == n_in
    pairs = [_meshes(c, i) for i in range(mb)]
    mo, mi = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])           # (mb, N, s), (mb, J, s)
    period = 0.0
    if metric == "euclid":
        m = orc.sqdist("euclid", mo, mi)                                                       # fp32 (mb, N, J)
    else:
        m = orc.sqdist(metric, mo[0], mi[0])[None]
        period = float(orc.period_1d(mi[0]) if metric == "periodic1d" else orc.period_2d(mi[0]))
    cvec = torch.tensor([1.7, 2.9, 2.2, 1.3][:H], dtype=torch.float32) * float(c.get("cmul", 2.0))
    mk, mk1, mmin = orc.row_order_stats(m, loc)
    _, w = orc.quantile_rank(loc, n_in)
    stats = torch.stack((mk, mk1, mmin)) if (masked or not self_attn) else None                  # (3, mb, N)
    if masked:
        T = torch.stack([orc.lerp_threshold(mk * cvec[h], mk1 * cvec[h], w) for h in range(H)], 1)  # (mb, H, N) fp32
    else:
        T = torch.full((mb, H, n_out), float("inf"))
    smin = torch.stack([(mmin * cvec[h]) if stats is not None else torch.zeros_like(mmin) for h in range(H)], 1)
    kept = torch.zeros(mb, n_out, dtype=torch.long)
    for h in range(H):                                                  # the 4-ulp condition (tests/test_gpu_att_edges.py)
        s, t = (m * cvec[h]).double(), T[:, h, :, None].double()
        if masked:
            ulp = torch.exp2(torch.floor(torch.log2(t.abs().clamp(min=1e-38))) - 23)
            dist = (s - t).abs()
            exact_tie = (dist == 0) & (mk == mk1)[..., None]
            assert bool(((dist > 4 * ulp) | exact_tie).all()), "a score within 4 ulp of its threshold: choose another seed"
            if c.get("dup"):
                assert bool(exact_tie.any()), "no exact tie at the threshold"
        kept = torch.maximum(kept, (s <= t).sum(-1))
    if metric != "euclid" and masked:                                   # rows 0..2 keep keys from across the wrap
        far = ((mo[0][:3, None, :] - mi[0][None, :, :]).abs() > 0.5).any(-1) & ((m[0, :3] * cvec[0]) <= T[0, 0, :3, None])
        assert bool(far.any(-1).all()), "a row at the wrap keeps no key from the other side"
    col0 = c.get("col0", 0)
    vals = torch.randn((b, n_in, dim), generator=torch.Generator().manual_seed(7 * seed + 1))
    dout = torch.randn((b, n_out, col0 + H * dim), generator=torch.Generator().manual_seed(7 * seed + 2))
    r64 = _evaluate(m, cvec, T, smin, vals, dout, col0, torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    return dict(mo=mo, mi=mi, m=m, vals=vals, cvec=cvec, dout=dout, T=T, smin=smin, kept=kept, r64=r64, w=w, stats=stats,
                period=period, masked=masked, mb=mb, col0=col0)


def _rb(t):
    return t.float().bfloat16().double()


@functools.lru_cache(maxsize=2)
def reference_bf16(key):
    """out and d(values) with both operands of every contraction rounded to bf16 (RNE) and fp64 accumulation: the forward contracts
    the un-normalised weights exp(S_min - s) with the values and scales by 1/L, d(values) contracts the normalised weights with d_out."""
    ref = reference(key)
    m, cvec, T, smin, V, dout, col0 = (ref[k] for k in ("m", "cvec", "T", "smin", "vals", "dout", "col0"))
    D, outs, dv = V.shape[-1], [], torch.zeros(V.shape, dtype=torch.float64)
    for h in range(cvec.numel()):
        s = m * cvec[h]
        a = torch.where(s <= T[:, h, :, None], torch.exp(smin[:, h, :, None].double() - s.double()), torch.zeros((), dtype=torch.float64))
        L = a.sum(-1, keepdim=True)
        outs.append(torch.matmul(_rb(a), _rb(V)) / L)
        dv += torch.matmul(_rb(a / L).transpose(-1, -2), _rb(dout[..., col0 + h * D: col0 + (h + 1) * D]))
    return dict(out=torch.cat(outs, -1), dv=dv)


def _lib_():
    from position_induced_transformer_amd import _lib
    return _lib


# --------------------------------------------------------------------------- the runner
class Run:
    """One case on the GPU: the guarded inputs, and one method per entry call."""

    def __init__(self, c):
        self.c = c
        self.geo = tuple(sorted((k, v) for k, v in c.items() if k in GEOMETRY))
        self.ref = ref = reference(self.geo)
        self.b, self.dim, self.H, self.mb = c["batch"], c["dim"], c["heads"], ref["mb"]
        self.n_out, self.n_in, self.sdim = c["n_out"], c["n_in"], ref["mo"].shape[-1]
        self.masked, self.self_attn, self.col0 = ref["masked"], bool(c.get("self_attn")), ref["col0"]
        self.width = self.col0 + self.H * self.dim
        self.mo = Buf(1, self.mb * self.n_out, self.sdim, data=ref["mo"])
        self.mi = self.mo if self.self_attn else Buf(1, self.mb * self.n_in, self.sdim, data=ref["mi"])
        self.stats = None if ref["stats"] is None else Buf(1, 1, 3 * self.mb * self.n_out, data=ref["stats"])
        self.head = Buf(1, 1, self.H, data=ref["cvec"])
        self.V = self._buf("v", self.b, self.n_in, self.dim, data=ref["vals"])
        print(f"  kept keys per row {int(ref['kept'].min())}..{int(ref['kept'].max())} of {self.n_in}")

    def _buf(self, who, b, rows, n, data=None):
        """A tensor of the case: pad / gap / off / skew of the case, `<who>pad` etc. override them for tensor `who` (v, o, d, dv)."""
        c = self.c
        get = lambda k, dflt: c.get(who + k, c.get(k, dflt))
        return SBuf(b, rows, n, get("pad", 4), get("gap", 4), get("off", 0), get("skew", 0), data=data)

    def _mesh(self):
        return (self.mo.ptr, self.mi.ptr, self.mb, self.n_out, self.n_in, self.sdim, METRIC[self.c.get("metric", "euclid")], self.ref["period"])

    def cols_view(self, t, heads):
        """(b, R, heads * D) -> the kernels' column space: (heads, R, b * D) on a shared mesh, (b * heads, R, D) per sample."""
        b, R, W = t.shape
        t = t.reshape(b, R, heads, W // heads)
        if self.mb == 1:
            return t.permute(2, 1, 0, 3).reshape(heads, R, b * (W // heads))
        return t.permute(0, 2, 1, 3).reshape(b * heads, R, W // heads)

    def _records(self, want, n_finish=0):
        got, att = dense_counts(), att_counts()
        print(f"  dense record {got}\n  expected     {want}\n  att record {att}")
        assert got == want
        n_dense = sum(v for k, v in want.items() if k in COUNTERS)
        want_att = {k: v for k, v in (("dhead_finish", n_finish), ("dense", n_dense)) if v}
        assert att == want_att

    # -- pit_posatt_fwd ---------------------------------------------------------------------------------------------------
    def forward(self, spec, mode=FP32, rc_want=0, copy=False, lmda=None, stats=True):
        L, ref = _lib_(), self.ref
        bf = (mode & 0xff) == BF16
        out = self._buf("o", self.b, self.n_out, self.width)
        rowstat, scale_out = Buf(1, self.mb * self.H * self.n_out, 4), Buf(1, 1, self.H)
        head = self.head if lmda is None else Buf(1, 1, self.H, data=lmda)
        dense_counts(), att_counts()
        rc = L.lib().pit_posatt_fwd(*self._mesh(), self.V.ptr, self.b, self.dim, self.V.ld, self.V.bs, head.ptr, self.H,
                                    1 if lmda is None else 0, self.stats.ptr if (self.stats is not None and stats) else None,
                                    ref["w"] if self.masked else 0.0, 1 if self.masked else 0, 1 if self.self_attn else 0,
                                    out.ptr, out.ld, out.bs, self.col0, 1 if copy else 0, rowstat.ptr, scale_out.ptr,
                                    None, None, 0, 0, mode, L.stream_ptr())
        torch.cuda.synchronize()
        print(f"  forward (mode {mode:#x}): rc {rc}")
        self._records(record(spec, self.masked, bf, "fwd") if not rc_want else {})
        assert rc == rc_want
        if rc:
            assert out.unwritten() and rowstat.unwritten() and scale_out.unwritten()
            return None
        assert self.V.untouched() and head.untouched() and self.mo.untouched() and self.mi.untouched()
        assert self.stats is None or self.stats.untouched()
        assert out.untouched() and rowstat.untouched() and scale_out.untouched()
        o, rs = out.cpu(), rowstat.cpu().view(self.mb, self.H, self.n_out, 4)
        assert bool(torch.isfinite(rs[..., 1:]).all()) and bool(torch.isfinite(o[..., self.col0:]).all())
        if copy:
            assert torch.equal(o[..., :self.dim], ref["vals"]), "copy_inputs: columns [0, dim)"
        elif self.col0:                               # columns below out_col0 belong to the caller: never written
            below = out.buf.as_strided(out.shape, out.strides, out.start)[..., :self.col0]
            assert bool((below == out.fill).all()), "wrote below out_col0"
        if lmda is not None:
            return scale_out
        o, r64 = self.cols_view(o[..., self.col0:], self.H), ref["r64"]
        assert torch.equal(rs[..., 0], ref["T"]) and torch.equal(rs[..., 1], ref["smin"]), "T / S_min not bit-equal"
        assert torch.equal(scale_out.cpu().view(-1), ref["cvec"])
        tag = "bf16" if bf else "fp32"
        if bf:
            compare_bf(f"out[{tag}]", o, self.cols_view(r64["out"], self.H), self.cols_view(reference_bf16(self.geo)["out"], self.H), TOL_BF["fwd"])
        else:
            compare(f"out[{tag}]", o, self.cols_view(r64["out"], self.H), TOL["fwd"], 32, 32)
        flat = lambda t: t.reshape(1, -1, 1)
        compare(f"1/L[{tag}]", flat(rs[..., 2]), flat(r64["invl"]), TOL["fwd"], 1, 1)
        compare(f"mbar[{tag}]", flat(rs[..., 3]), flat(r64["mbar"]), TOL["fwd"], 1, 1)
        return scale_out

    # -- pit_posatt_bwd ---------------------------------------------------------------------------------------------------
    def backward(self, spec, want_dv, want_dc, mode=FP32, rc_want=0, resid=False, acc=0, rider=None, dhead0=None):
        """d(values) and / or d(c) from the reference's rowstat (fp32 roundings of the fp64 1/L and mbar, the exact T and S_min).
        Returns (work, dhead) of a deferred call."""
        L, ref = _lib_(), self.ref
        bf = (mode & 0xff) == BF16
        dout = self._buf("d", self.b, self.n_out, self.width, data=ref["dout"])
        rsd = torch.stack((ref["T"], ref["smin"], ref["r64"]["invl"].float(), ref["r64"]["mbar"].float()), -1)
        rowstat = Buf(1, self.mb * self.H * self.n_out, 4, data=rsd)
        dvb = self._buf("dv", self.b, self.n_in, self.dim) if want_dv else None
        dhead = Buf(1, 1, self.H, data=dhead0) if want_dc else None
        work = torch.zeros(self.H * SLOTS, dtype=torch.float64, device="cuda")
        dense_counts(), att_counts()
        rc = L.lib().pit_posatt_bwd(*self._mesh(), self.V.ptr, self.b, self.dim, self.V.ld, self.V.bs, self.head.ptr, self.H, 1, None,
                                    rowstat.ptr, 1 if self.masked else 0, dout.ptr, dout.ld, dout.bs, self.col0,
                                    dvb.ptr if dvb else None, dvb.ld if dvb else 0, dvb.bs if dvb else 0, 1 if resid else 0,
                                    dhead.ptr if dhead else None, acc, work.data_ptr(), None, None, 0, 0, None, None, rider,
                                    0, mode, L.stream_ptr())
        torch.cuda.synchronize()
        print(f"  backward (mode {mode:#x}, d(values) {want_dv}, d(c) {want_dc}): rc {rc}")
        defer = bool(acc & HEAD_DEFER)
        self._records(record(spec, self.masked, bf, "dscale") if not rc_want else {}, 1 if (want_dc and not defer and not rc_want) else 0)
        assert rc == rc_want
        assert dout.untouched() and rowstat.untouched() and self.V.untouched() and self.head.untouched()
        assert self.mo.untouched() and self.mi.untouched()
        if rc:
            assert (dvb is None or dvb.unwritten()) and (dhead is None or dhead0 is not None or dhead.unwritten())
            assert float(work.abs().max()) == 0.0
            return None
        r64, tag = ref["r64"], "bf16" if bf else "fp32"
        if dvb is not None:
            assert dvb.untouched()
            want = r64["dv"] + (ref["dout"][..., :self.dim].double() if resid else 0.0)
            if bf:
                emu = reference_bf16(self.geo)["dv"] + (ref["dout"][..., :self.dim].double() if resid else 0.0)
                compare_bf(f"d(values)[{tag}]", self.cols_view(dvb.cpu(), 1), self.cols_view(want, 1), self.cols_view(emu, 1), TOL_BF["dv"])
            else:
                compare(f"d(values)[{tag}]", self.cols_view(dvb.cpu(), 1), self.cols_view(want, 1), TOL["dv"], 32, 32)
        if defer:
            assert dhead is None or dhead0 is not None or dhead.unwritten()
            return work, dhead
        assert float(work.abs().max()) == 0.0, "the fp64 d(scale) accumulators are not left zero"
        if dhead is not None:
            assert dhead.untouched()
            want = r64["dc"] + (dhead0.double() if (acc & HEAD_ACCUMULATE) else 0.0)
            compare(f"d(c)[{tag}]", dhead.cpu(), want.reshape(1, 1, -1), TOL["dc"], 1, 1)
        return None


def _case(id_, n_out, n_in, batch, dim, heads, **kw):
    return pytest.param(dict(n_out=n_out, n_in=n_in, batch=batch, dim=dim, heads=heads, **kw), id=id_)


def _both(cases, seeds):
    """Every geometry unmasked and masked (locality 0.3, 0.2 from 257 keys on); `seeds`: where seed 1 misses the 4-ulp condition."""
    out = []
    for p in cases:
        c = p.values[0]
        out += [p, pytest.param(dict(c, loc=0.2 if c["n_in"] >= 257 else 0.3, seed=seeds.get(p.id, 1)), id=p.id + "-masked")]
    return out


# --------------------------------------------------------------------------- J-split rows: every (CT, waves)
# rows = (CT, waves, IL) of posatt_rows_kernel, grid = (mesh_batch * column groups, heads, row tiles).  CT 1: a shared mesh with
# ncols = batch * dim of 96 / 140 / 5; CT 2: per-sample meshes of 192 / 190 columns (16 samples fill 256 workgroups); CT 4: per-sample
# meshes of 512 / 500 columns, 8 samples, 2 heads, 4 row tiles (exactly 256 workgroups).  waves = pow2_floor(n_in / 32), n_in never a
# multiple of waves * 2 * NP (NP 8, CT 4: 4): the last wave's slice is partial, and at 257 keys on 8 waves the last two have none.
ROWS = _both([
    _case("rows-ct1-w1-33keys", 70, 33, 2, 48, 1, rows=(1, 1, 0), grid=(3, 1, 3)),
    _case("rows-ct1-w2-3heads-dim70", 45, 70, 2, 70, 3, rows=(1, 2, 0), grid=(5, 3, 2)),
    _case("rows-ct1-w4-dim1", 33, 130, 5, 1, 2, rows=(1, 4, 0), grid=(1, 2, 2)),
    _case("rows-ct1-w8-empty-waves", 64, 257, 2, 48, 1, rows=(1, 8, 0), grid=(3, 1, 2)),
    _case("rows-ct2-w1", 170, 33, 8, 192, 2, per_sample=True, rows=(2, 1, 0), grid=(24, 2, 6)),
    _case("rows-ct2-w2-190cols", 170, 100, 8, 190, 2, per_sample=True, rows=(2, 2, 0), grid=(24, 2, 6)),
    _case("rows-ct2-w4", 170, 130, 8, 192, 2, per_sample=True, rows=(2, 4, 0), grid=(24, 2, 6)),
    _case("rows-ct2-w8-190cols", 170, 257, 8, 190, 2, per_sample=True, rows=(2, 8, 0), grid=(24, 2, 6)),
    _case("rows-ct4-w1", 128, 33, 8, 512, 2, per_sample=True, rows=(4, 1, 1), grid=(32, 2, 4)),
    _case("rows-ct4-w2-500cols-120rows", 120, 100, 8, 500, 2, per_sample=True, rows=(4, 2, 1), grid=(32, 2, 4)),
    _case("rows-ct4-w4", 128, 257, 8, 512, 2, per_sample=True, rows=(4, 4, 1), grid=(32, 2, 4)),
], seeds={"rows-ct2-w8-190cols": 2})


@pytest.mark.parametrize("c", ROWS)
def test_jsplit_rows_by_instance(c):
    """posatt_rows_kernel<CT, MODE, M, BF, IL>: forward in fp32 and in bf16 math, d(scale) alone."""
    r = Run(c)
    spec = dict(rows=c["rows"], grid=c["grid"])
    r.forward(spec)
    r.forward(spec, mode=BF16)
    r.backward(spec, False, True)
    r.backward(spec, False, True, mode=BF16)                # (bf16 math asked for: d(scale) stays on the fp32 instance and bound)


# --------------------------------------------------------------------------- J-split cols: every (CT, waves)
# cols = (CT, waves, IL) of posatt_cols_kernel, grid = (column groups, key tiles, mesh_batch); waves = pow2_floor(n_out * heads / 32)
COLS = _both([
    _case("cols-ct1-w1", 33, 70, 2, 48, 1, cols=(1, 1, 0), grid=(3, 3, 1)),
    _case("cols-ct1-w2-dim70", 45, 70, 2, 70, 2, cols=(1, 2, 0), grid=(5, 3, 1)),
    _case("cols-ct1-w4-3heads-dim1", 50, 100, 5, 1, 3, cols=(1, 4, 0), grid=(1, 4, 1)),
    _case("cols-ct1-w8", 257, 64, 2, 48, 1, cols=(1, 8, 0), grid=(3, 2, 1)),
    _case("cols-ct2-w1", 33, 170, 16, 192, 1, per_sample=True, cols=(2, 1, 0), grid=(3, 6, 16)),
    _case("cols-ct2-w2-190cols", 70, 170, 16, 190, 1, per_sample=True, cols=(2, 2, 0), grid=(3, 6, 16)),
    _case("cols-ct2-w4", 70, 170, 16, 192, 2, per_sample=True, cols=(2, 4, 0), grid=(3, 6, 16)),
    _case("cols-ct2-w8", 130, 170, 16, 192, 2, per_sample=True, cols=(2, 8, 0), grid=(3, 6, 16)),
    _case("cols-ct4-w1", 33, 257, 8, 512, 1, per_sample=True, cols=(4, 1, 1), grid=(4, 9, 8)),
    _case("cols-ct4-w2-500cols", 70, 257, 8, 500, 1, per_sample=True, cols=(4, 2, 1), grid=(4, 9, 8)),
    _case("cols-ct4-w4", 120, 257, 8, 512, 2, per_sample=True, cols=(4, 4, 1), grid=(4, 9, 8)),
], seeds={"cols-ct4-w1": 2})


@pytest.mark.parametrize("c", COLS)
def test_jsplit_cols_by_instance(c):
    """posatt_cols_kernel<CT, M, BF, IL>: d(values) alone in fp32 and in bf16 math."""
    r = Run(c)
    spec = dict(cols=c["cols"], grid=c["grid"])
    r.backward(spec, True, False)
    r.backward(spec, True, False, mode=BF16)


# --------------------------------------------------------------------------- interleaved tiles and their twins
# One shape (8 per-sample meshes, 128 rows, 257 keys, 2 heads, dim 512: CT 4, 4 waves in all three launches) and one declining
# condition at a time; `decl` = the interleave_ok modes (0 forward, 1 d(scale), 2 d(values)) the condition switches to IL = false.
IL = [
    _case("il-all-interleaved", 128, 257, 8, 512, 2, per_sample=True, decl=()),
    _case("il-values-4-bytes-off", 128, 257, 8, 512, 2, per_sample=True, voff=1, decl=(0, 1)),
    _case("il-out-4-bytes-off", 128, 257, 8, 512, 2, per_sample=True, ooff=1, decl=(0,)),
    _case("il-dout-4-bytes-off", 128, 257, 8, 512, 2, per_sample=True, doff=1, decl=(1, 2)),
    _case("il-dvalues-4-bytes-off", 128, 257, 8, 512, 2, per_sample=True, dvoff=1, decl=(2,)),
    _case("il-ld-values-not-4", 128, 257, 8, 512, 2, per_sample=True, vpad=5, vskew=3, decl=(0, 1)),      # (261 * 517 + 3: the sample stride stays a multiple of 4)
    _case("il-ld-dvalues-not-4", 128, 257, 8, 512, 2, per_sample=True, dvpad=6, dvskew=2, decl=(2,)),     # (261 * 518 + 2)
    _case("il-out-sample-stride-not-4", 128, 257, 8, 512, 2, per_sample=True, oskew=2, decl=(0,)),
    _case("il-dout-sample-stride-not-4", 128, 257, 8, 512, 2, per_sample=True, dskew=1, decl=(1, 2)),
    _case("il-out-col0-not-4", 128, 257, 8, 512, 2, per_sample=True, col0=2, pad=2, vpad=4, dvpad=4, decl=(0, 1, 2)),
    _case("il-dim-not-4", 128, 257, 8, 510, 2, per_sample=True, pad=2, opad=4, dpad=4, decl=(0, 1, 2)),    # (every ld a multiple of 4: 512, 1024)
    _case("il-masked-interleaved", 128, 257, 8, 512, 2, per_sample=True, loc=0.2, decl=()),
    _case("il-masked-values-4-bytes-off", 128, 257, 8, 512, 2, per_sample=True, loc=0.2, voff=1, decl=(0, 1)),
]


@pytest.mark.parametrize("c", IL)
def test_interleaved_tiles_and_their_twins(c):
    """IL = true (16-byte loads and stores over columns {4 l + t}) against IL = false on the same shape and data: the record says
    which twin ran, both meet the bounds."""
    r = Run(c)
    il = [0 if mode in c["decl"] else 1 for mode in (0, 1, 2)]
    r.forward(dict(rows=(4, 4, il[0]), grid=(32, 2, 4)))
    r.forward(dict(rows=(4, 4, il[0]), grid=(32, 2, 4)), mode=BF16)
    r.backward(dict(rows=(4, 4, il[1]), grid=(32, 2, 4)), False, True)
    r.backward(dict(cols=(4, 4, il[2]), grid=(4, 9, 8)), True, False)
    r.backward(dict(cols=(4, 4, il[2]), grid=(4, 9, 8)), True, False, mode=BF16)


# --------------------------------------------------------------------------- chunk seams
CHUNK_KEYS = [
    _case("chunk-keys-2048", 70, 2048, 2, 16, 1, cmul=0.5, j_tiles=64),
    _case("chunk-keys-2049", 70, 2049, 2, 16, 1, cmul=0.5, j_tiles=65),
    _case("chunk-keys-2080", 70, 2080, 2, 16, 1, cmul=0.5, j_tiles=65),
    _case("chunk-keys-2049-masked", 70, 2049, 2, 16, 1, loc=0.4, cmul=0.5, j_tiles=65),
]


@pytest.mark.parametrize("c", CHUNK_KEYS)
def test_key_chunk_seam(c):
    """n_in across KEY_CHUNK = 2048: the second pass of the rows kernel holds 0, 1 or 32 keys (all but the first wave idle at 1);
    the cols and pair kernels get a 65th key tile."""
    r = Run(c)
    rows, cols = dict(rows=(1, 8, 0), grid=(1, 1, 3)), dict(cols=(1, 2, 0), grid=(1, c["j_tiles"], 1))
    r.forward(rows)
    r.forward(rows, mode=BF16)
    r.backward(rows, False, True)
    r.backward(cols, True, False)
    r.backward(dict(pair=(1, 2, 0), grid=(3 + c["j_tiles"], 1, 1)), True, True)


CHUNK_ROWS = [
    _case("chunk-rows-1024", 1024, 40, 2, 16, 1, n_tiles=32),
    _case("chunk-rows-1025", 1025, 40, 2, 16, 1, n_tiles=33),
    _case("chunk-rows-1025-masked-2heads", 1025, 40, 2, 16, 2, loc=0.4, n_tiles=33),
]


@pytest.mark.parametrize("c", CHUNK_ROWS)
def test_row_chunk_seam(c):
    """n_out across ROW_CHUNK = 1024 in the cols kernel (alone and inside the pair): the second pass holds 0 or 1 rows."""
    r = Run(c)
    H = c["heads"]
    r.forward(dict(rows=(1, 1, 0), grid=(1, H, c["n_tiles"])))
    r.backward(dict(cols=(1, 8, 0), grid=(1, 2, 1)), True, False)
    r.backward(dict(cols=(1, 8, 0), grid=(1, 2, 1)), True, False, mode=BF16)
    r.backward(dict(pair=(1, 1, 0), grid=(H * c["n_tiles"] + 2, 1, 1)), True, True)


# --------------------------------------------------------------------------- the merged backward
# pair = (CT, waves, IL); grid.x = rows workgroups + cols workgroups (the cols workgroups come first in the id space)
PAIR = [
    _case("pair-ct1-3heads-shared", 70, 100, 2, 48, 3, pair=(1, 2, 0), grid=(39, 1, 1)),
    _case("pair-ct1-3heads-per-sample-masked", 45, 70, 3, 70, 3, per_sample=True, loc=0.3, pair=(1, 2, 0), grid=(81, 1, 1)),
    _case("pair-ct2", 170, 170, 16, 192, 2, per_sample=True, pair=(2, 4, 0), grid=(864, 1, 1)),
    _case("pair-ct2-masked-190cols", 170, 170, 16, 190, 2, per_sample=True, loc=0.3, pair=(2, 4, 0), grid=(864, 1, 1)),
    _case("pair-ct4-il", 128, 257, 8, 512, 2, per_sample=True, pair=(4, 4, 1), grid=(544, 1, 1)),
    _case("pair-ct4-il-masked", 128, 257, 8, 512, 2, per_sample=True, loc=0.2, pair=(4, 4, 1), grid=(544, 1, 1)),
    _case("pair-ct4-no-il", 128, 257, 8, 512, 2, per_sample=True, doff=1, pair=(4, 4, 0), grid=(544, 1, 1)),
]


@pytest.mark.parametrize("c", PAIR)
def test_merged_backward_by_instance(c):
    """d(scale) + d(values) in one launch: posatt_bwd_pair_kernel (CT 1), posatt_bwd_pair_wide_kernel (CT 2, CT 4 with and without
    IL); bf16 math runs the cols half in bf16 and the rows half in fp32."""
    r = Run(c)
    spec = dict(pair=c["pair"], grid=c["grid"])
    r.backward(spec, True, True)
    r.backward(spec, True, True, mode=BF16)


def test_merged_backward_declined_when_rows_and_cols_choose_another_ct():
    """8 samples x 128 rows x 2 heads x 512 columns against 100 keys: 64 row tiles fill the chip at CT 4, 32 key tiles only at CT 2
    - two launches, the result is still right."""
    r = Run(dict(n_out=128, n_in=100, batch=8, dim=512, heads=2, per_sample=True))
    r.backward(dict(rows=(4, 2, 1), cols=(2, 8, 0), grid=(8, 4, 8)), True, True)


@pytest.mark.parametrize("n_in,paired", [(288, True), (289, False)])
def test_merged_backward_workgroup_limit(n_in, paired):
    """32 samples x 3 column groups: 3168 rows workgroups (11 row tiles x 3 heads) + 864 cols workgroups (9 key tiles) = 4032 are
    merged, a tenth key tile makes 4128 > 4096 and the two launches run separately."""
    r = Run(dict(n_out=352, n_in=n_in, batch=32, dim=96, heads=3, per_sample=True))
    if paired:
        r.backward(dict(pair=(1, 8, 0), grid=(4032, 1, 1)), True, True)
    else:
        r.backward(dict(rows=(1, 8, 0), cols=(1, 8, 0), grid=(3, 10, 32)), True, True)


RIDER_DW_WGS, RIDER_WIDE_WGS = 4, 4          # workgroups the Rider of tests/test_gpu_att_edges.py (256 rows, 24 -> 16 -> 8) adds


def test_merged_backward_carrying_riders():
    """A postponed weight-gradient job inside posatt_bwd_pair_dw_kernel (CT 1, >= 2 waves) and as gemm_rr_tile tiles behind the
    workgroups of posatt_bwd_pair_wide_kernel (CT 2, >= 4 waves): the record and the attention result (the GEMMs are
    tests/test_gpu_riders.py's)."""
    r = Run(dict(n_out=70, n_in=100, batch=2, dim=48, heads=3))
    rd = Rider()
    r.backward(dict(pair=(1, 2, 0), pair_kind="pair_dw", grid=(39 + RIDER_DW_WGS, 1, 1)), True, True, rider=rd.ptr)
    assert rd.delivered()
    r = Run(dict(n_out=170, n_in=170, batch=16, dim=192, heads=2, per_sample=True))
    rd = Rider()
    r.backward(dict(pair=(2, 4, 0), grid=(864 + RIDER_WIDE_WGS, 1, 1)), True, True, rider=rd.ptr)
    assert rd.delivered()


# --------------------------------------------------------------------------- the large-regime kernels
# PIT_FORCE_TILES=1 and PIT_FORCE_RT (both read per call).  S = a shared mesh, batch 4 x dim 64 = 256 columns (8 column tiles: tpwg 8),
# 100 rows, 2 heads; G = 16 per-sample meshes of 544 columns (17 column tiles: tpwg 16, the second workgroup of a row holds ONE
# tile - tile_end cuts its waves' lists), 257 rows, 4 heads; W = 16 per-sample meshes of 1024 columns (tpwg 32), 257 rows, 4 heads.
# trows = (RT, TPWG), grid = (mesh_batch * column groups, heads, row-tile groups).
def _tiles(id_, n_in, rt, shape, **kw):
    n_out, batch, dim, heads, per, tpwg, cg = dict(S=(100, 4, 64, 2, False, 8, 1), G=(257, 16, 544, 4, True, 16, 2),
                                                   W=(257, 16, 1024, 4, True, 32, 1))[shape]
    n_tiles = (n_out + 31) // 32
    grid = ((batch if per else 1) * cg, heads, (n_tiles + rt - 1) // rt)
    return _case(id_, n_out, n_in, batch, dim, heads, per_sample=per, rt=rt, trows=(rt, tpwg), grid=grid, **kw)


TILES_ROWS = [
    _tiles("tiles-r1x1-255keys", 255, 1, "S"),
    _tiles("tiles-r1x1-256keys-masked", 256, 1, "S", loc=0.3),
    _tiles("tiles-r1x1-257keys", 257, 1, "S"),
    _tiles("tiles-r1x1-257keys-masked", 257, 1, "S", loc=0.3),
    _tiles("tiles-r2x1-129keys", 129, 2, "S"),
    _tiles("tiles-r2x1-256keys-masked", 256, 2, "S", loc=0.3),
    _tiles("tiles-r4x1-65keys-masked", 65, 4, "S", loc=0.3),
    _tiles("tiles-r4x1-256keys", 256, 4, "S"),
    _tiles("tiles-r1x2-100keys-17coltiles", 100, 1, "G"),
    _tiles("tiles-r1x2-100keys-17coltiles-masked", 100, 1, "G", loc=0.3),
    _tiles("tiles-r2x2-129keys-17coltiles", 129, 2, "G"),
    _tiles("tiles-r2x2-129keys-17coltiles-masked", 129, 2, "G", loc=0.3),
    _tiles("tiles-r1x4-100keys", 100, 1, "W"),
    _tiles("tiles-r1x4-100keys-masked", 100, 1, "W", loc=0.3),
]


@pytest.mark.parametrize("c", TILES_ROWS)
def test_rows_tiles_by_instance(c, monkeypatch):
    """posatt_rows_tiles<RT, TPW, MODE, M, BF, false>: forward fp32 / bf16 and d(scale), key counts at the KC = 256 / RT seams."""
    monkeypatch.setenv("PIT_FORCE_TILES", "1")
    monkeypatch.setenv("PIT_FORCE_RT", str(c["rt"]))
    r = Run(c)
    spec = dict(trows=c["trows"], grid=c["grid"])
    r.forward(spec)
    r.forward(spec, mode=BF16)
    r.backward(spec, False, True)


TILES_COLS = [
    _case("tiles-cols-8-100rows", 100, 257, 4, 64, 2, tcols=8, grid=(1, 9, 1)),
    _case("tiles-cols-8-255rows-masked", 255, 100, 4, 64, 2, loc=0.3, tcols=8, grid=(1, 4, 1)),
    _case("tiles-cols-8-256rows", 256, 100, 4, 64, 1, tcols=8, grid=(1, 4, 1)),
    _case("tiles-cols-8-257rows-masked", 257, 100, 4, 64, 1, loc=0.3, tcols=8, grid=(1, 4, 1)),
    _case("tiles-cols-16-17coltiles", 100, 500, 16, 544, 1, per_sample=True, tcols=16, grid=(2, 16, 16)),
    _case("tiles-cols-16-17coltiles-masked", 100, 500, 16, 544, 1, per_sample=True, loc=0.3, tcols=16, grid=(2, 16, 16)),
    _case("tiles-cols-32", 70, 1000, 16, 1024, 1, per_sample=True, tcols=32, grid=(1, 32, 16)),
    _case("tiles-cols-32-masked", 70, 1000, 16, 1024, 1, per_sample=True, loc=0.3, seed=2, tcols=32, grid=(1, 32, 16)),
]


@pytest.mark.parametrize("c", TILES_COLS)
def test_cols_tiles_by_instance(c, monkeypatch):
    """posatt_cols_tiles<TPW, M, BF, false> at 8, 16 and 32 column tiles per workgroup, row counts at the TK_CHUNK = 256 seam."""
    monkeypatch.setenv("PIT_FORCE_TILES", "1")
    r = Run(c)
    spec = dict(tcols=c["tcols"], grid=c["grid"])
    r.backward(spec, True, False)
    r.backward(spec, True, False, mode=BF16)


@pytest.mark.parametrize("n_in,rows_tiles", [(1024, True), (1022, False)])
def test_work_threshold_of_the_tiles_regime_unforced(n_in, rows_tiles):
    """A shared mesh, 1 head, 1024 rows, 16 x 64 = 1024 columns: 1024 keys are exactly 2^19 units of work (the tiles kernels), 1022
    keys are 523 264 (the J-split kernels: CT 4, 4 waves, interleaved) while the cols launch (work from n_out) stays on the tiles
    kernels - and the merged backward declines because one part is in the tiles regime."""
    r = Run(dict(n_out=1024, n_in=n_in, batch=16, dim=64, heads=1, cmul=8.0))
    if rows_tiles:
        r.forward(dict(trows=(1, 8), grid=(4, 1, 32)))
        r.backward(dict(trows=(1, 8), tcols=8, grid=(4, 32, 1)), True, True)
    else:
        r.forward(dict(rows=(4, 4, 1), grid=(8, 1, 32)))
        r.backward(dict(rows=(4, 4, 1), tcols=8, grid=(4, 32, 1)), True, True)


# --------------------------------------------------------------------------- precomputed weights
class Pre:
    """pit_posatt_pre_fwd / _bwd on E, Q and rowstat from ops.block_weights (inputs here); the fp64 references are formed from
    those fp32 values: out_h = (E_h / rowsum_h) V, d(values) = residual + sum_h (E_h / rowsum_h)^T dO_h, d c_h = -<V, Q_h^T dO_h>."""

    def __init__(self, n_pts, batch, dim, heads, seed=1, **strides):
        from position_induced_transformer_amd import ops
        self.n, self.b, self.dim, self.H, self.s = n_pts, batch, dim, heads, strides
        mesh = lattice(n_pts, 2, 100 * seed)
        if n_pts % 4 == 0 and n_pts <= 2048:
            plan = ops.MeshPlan("euclid", mesh.cuda(), mesh.cuda(), 1.0, True)
            lmda = torch.tensor([0.3, -0.7][:heads], device="cuda")
            E, Q, _inv, rowstat, scale, _ = ops.block_weights(plan, [lmda], heads)
            torch.cuda.synchronize()
        else:                   # pit_block_weights takes multiples of 4 up to 2048 only: the same quantities from the CPU, full-sized, for a refusal
            m, c = orc.sqdist("euclid", mesh, mesh), torch.tensor([1.9, 0.7][:heads])
            e = torch.exp(-c[:, None, None] * m)
            rsum = e.sum(-1)
            mbar = (e * m).sum(-1) / rsum
            q = e * (m - mbar[..., None]) / rsum[..., None]
            rs = torch.stack((torch.full_like(rsum, float("inf")), torch.zeros_like(rsum), 1.0 / rsum, mbar), -1)
            E, Q, rowstat, scale = e[None], q[None], rs[None], c[None]
        self.e64, self.q64, self.rs = E[0].double().cpu(), Q[0].double().cpu(), rowstat[0].cpu()
        self.E = Buf(1, heads * n_pts, n_pts, data=E[0])
        self.Q = Buf(1, heads * n_pts, n_pts, data=Q[0])
        self.rowstat = Buf(1, heads * n_pts, 4, data=rowstat[0])
        self.head = Buf(1, 1, heads, data=scale[0])
        g = torch.Generator().manual_seed(7 * seed + 1)
        self.vals, self.dout = torch.randn((batch, n_pts, dim), generator=g), torch.randn((batch, n_pts, (1 + heads) * dim), generator=g)
        self.V = SBuf(batch, n_pts, dim, 4, 4, data=self.vals)
        invl = self.rs[..., 2].double()                                       # (H, n)
        P = self.e64 * invl[..., None]
        V, g_ = self.vals.double(), [self.dout[..., (1 + h) * dim:(2 + h) * dim].double() for h in range(heads)]
        self.out64 = torch.cat([torch.matmul(P[h], V) for h in range(heads)], -1)
        self.dv64 = sum(torch.matmul(P[h].T, g_[h]) for h in range(heads))
        self.dc64 = torch.stack([-(g_[h] * torch.matmul(self.q64[h], V)).sum() for h in range(heads)])
        self.out_bf = torch.cat([torch.matmul(_rb(self.e64[h]), _rb(V)) * invl[h][:, None] for h in range(heads)], -1)
        self.dv_bf = sum(torch.matmul(_rb(P[h]).T, _rb(g_[h])) for h in range(heads))

    def view(self, t, heads):
        b, R, W = t.shape
        return t.reshape(b, R, heads, W // heads).permute(2, 1, 0, 3).reshape(heads, R, b * (W // heads))

    def _records(self, want):
        got, att = dense_counts(), att_counts()
        print(f"  dense record {got}\n  expected     {want}\n  att record {att}")
        assert got == want and att == {}

    def forward(self, spec, mode=FP32, copy=True, rc_want=0):
        L, n, H, dim = _lib_(), self.n, self.H, self.dim
        out = SBuf(self.b, n, (1 + H) * dim, 4, 4)
        dense_counts(), att_counts()
        rc = L.lib().pit_posatt_pre_fwd(self.E.ptr, self.rowstat.ptr, n, H, dim, self.b, self.V.ptr, self.V.ld, self.V.bs,
                                        out.ptr, out.ld, out.bs, dim, 1 if copy else 0, mode, L.stream_ptr())
        torch.cuda.synchronize()
        print(f"  pre forward (mode {mode:#x}): rc {rc}")
        self._records(record(spec, False, mode == BF16, "fwd", pre=True) if not rc_want else {})
        assert rc == rc_want
        assert self.E.untouched() and self.rowstat.untouched() and self.V.untouched()
        if rc:
            assert out.unwritten()
            return
        assert out.untouched()
        o = out.cpu()
        if copy:
            assert torch.equal(o[..., :dim], self.vals), "copy_inputs: columns [0, dim)"
        else:
            assert bool((out.buf.as_strided(out.shape, out.strides, out.start)[..., :dim] == out.fill).all()), "wrote below out_col0"
        if mode == BF16:
            compare_bf("pre out[bf16]", self.view(o[..., dim:], H), self.view(self.out64, H), self.view(self.out_bf, H), TOL_BF["fwd"])
        else:
            compare("pre out[fp32]", self.view(o[..., dim:], H), self.view(self.out64, H), TOL["fwd"], 32, 32)

    def backward(self, spec, mode=FP32, resid=True, dscale=True, rc_want=0):
        L, n, H, dim = _lib_(), self.n, self.H, self.dim
        dout = SBuf(self.b, n, (1 + H) * dim, 4, 4, data=self.dout)
        dvb = SBuf(self.b, n, dim, 4, 4)
        work = torch.zeros(H * SLOTS, dtype=torch.float64, device="cuda")
        dense_counts(), att_counts()
        rc = L.lib().pit_posatt_pre_bwd(self.E.ptr, self.Q.ptr, self.rowstat.ptr, n, H, dim, self.b, self.V.ptr, self.V.ld, self.V.bs,
                                        dout.ptr, dout.ld, dout.bs, dim, dvb.ptr, dvb.ld, dvb.bs, 1 if resid else 0,
                                        work.data_ptr() if dscale else None, mode, L.stream_ptr())
        torch.cuda.synchronize()
        print(f"  pre backward (mode {mode:#x}, residual {resid}, d(scale) {dscale}): rc {rc}")
        self._records(record(spec, False, mode == BF16, "dscale", pre=True) if not rc_want else {})
        assert rc == rc_want
        assert self.E.untouched() and self.Q.untouched() and self.rowstat.untouched() and self.V.untouched() and dout.untouched()
        if rc:
            assert dvb.unwritten() and float(work.abs().max()) == 0.0
            return
        assert dvb.untouched()
        want = self.dv64 + (self.dout[..., :dim].double() if resid else 0.0)
        if mode == BF16:
            emu = self.dv_bf + (self.dout[..., :dim].double() if resid else 0.0)
            compare_bf("pre d(values)[bf16]", self.view(dvb.cpu(), 1), self.view(want, 1), self.view(emu, 1), TOL_BF["dv"])
        else:
            compare("pre d(values)[fp32]", self.view(dvb.cpu(), 1), self.view(want, 1), TOL["dv"], 32, 32)
        if not dscale:
            assert float(work.abs().max()) == 0.0
            return
        dhead = Buf(1, 1, H)                          # the PIT_HEAD_DEFER convention: drain with pit_posatt_dhead_finish
        arr = lambda v: (ctypes.c_void_p * 1)(v)
        rc = L.lib().pit_posatt_dhead_finish(1, arr(work.data_ptr()), arr(dhead.ptr), arr(self.head.ptr), arr(self.head.ptr),
                                             (ctypes.c_int * 1)(H), (ctypes.c_int * 1)(HEAD_IS_SCALE), None, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and float(work.abs().max()) == 0.0 and dhead.untouched()
        compare(f"pre d(c)[{'bf16' if mode == BF16 else 'fp32'}]", dhead.cpu(), self.dc64.reshape(1, 1, -1), TOL["dc"], 1, 1)


def test_precomputed_weights_smallest_unforced_shape():
    """768 points x hid 256 x batch 4, two heads (tests/test_gpu_grad_delivery.py): the smallest shape pit_posatt_pre_supported
    accepts; rows and cols on the PRE instances at 8 column tiles per workgroup."""
    L = _lib_()
    assert L.lib().pit_posatt_pre_supported(768, 2, 256, 4) == 1
    p = Pre(768, 4, 256, 2)
    p.forward(dict(trows=(1, 8), grid=(4, 2, 24)))
    p.forward(dict(trows=(1, 8), grid=(4, 2, 24)), mode=BF16, copy=False)
    p.backward(dict(tcols=8, trows=(1, 8), grid=(4, 2, 24)))
    p.backward(dict(tcols=8, trows=(1, 8), grid=(4, 2, 24)), mode=BF16, resid=False)
    p.backward(dict(tcols=8, grid=(4, 24, 1)), dscale=False)


@pytest.mark.parametrize("rt", [1, 2, 4])
def test_precomputed_weights_forced_small_shapes(rt, monkeypatch):
    """100 points (a multiple of 4, not of 32) x 4 x 64 columns, one or two heads, forced into the tiles regime at RT 1, 2 and 4."""
    monkeypatch.setenv("PIT_FORCE_TILES", "1")
    monkeypatch.setenv("PIT_FORCE_RT", str(rt))
    heads = 1 if rt == 2 else 2
    p = Pre(100, 4, 64, heads, seed=2)
    g = (1, heads, (4 + rt - 1) // rt)
    p.forward(dict(trows=(rt, 8), grid=g))
    p.forward(dict(trows=(rt, 8), grid=g), mode=BF16)
    p.backward(dict(tcols=8, trows=(rt, 8), grid=g))
    p.backward(dict(tcols=8, grid=(1, 4, 1)), mode=BF16, dscale=False, resid=False)


# 100 points against very many columns (one head): with 4 row / key tiles the forced regime takes 16 column tiles per workgroup from
# 2033 column tiles on and 32 from 4065 on (tiles_per_wg_for: units * ceil(ntiles / tpwg) >= 512); RT 2 halves the rows units and is
# clamped to 16.  trows = (RT, TPWG), tcols = TPWG; grids (column groups, heads, row-tile groups) / (column groups, key tiles, 1).
PRE_WIDE = [
    pytest.param(dict(batch=16, dim=4096, rt=1, trows=(1, 16), tcols=16, cg=128), id="pre-r1x2-cols16-65536cols"),
    pytest.param(dict(batch=32, dim=4096, rt=1, trows=(1, 32), tcols=32, cg=128), id="pre-r1x4-cols32-131072cols"),
    pytest.param(dict(batch=32, dim=4096, rt=2, trows=(2, 16), tcols=32, cg=256), id="pre-r2x2-cols32-131072cols"),
]


@pytest.mark.parametrize("c", PRE_WIDE)
def test_precomputed_weights_many_column_tiles_per_workgroup(c, monkeypatch):
    """posatt_rows_tiles<1, 2 | 4, MODE, false, BF, true>, <2, 2, ...> and posatt_cols_tiles<2 | 4, false, BF, true>: the PRE instances
    beyond 8 column tiles per workgroup, forward and backward in fp32 and bf16 math."""
    monkeypatch.setenv("PIT_FORCE_TILES", "1")
    monkeypatch.setenv("PIT_FORCE_RT", str(c["rt"]))
    p = Pre(100, c["batch"], c["dim"], 1, seed=2)
    g = (c["cg"], 1, 4 // c["rt"])
    p.forward(dict(trows=c["trows"], grid=g))
    p.forward(dict(trows=c["trows"], grid=g), mode=BF16, copy=False)
    p.backward(dict(tcols=c["tcols"], trows=c["trows"], grid=g))
    p.backward(dict(tcols=c["tcols"], grid=(c["batch"] * c["dim"] // 32 // c["tcols"], 4, 1)), mode=BF16, dscale=False, resid=False)


def test_precomputed_weights_refusals(monkeypatch):
    """A shape outside the regime, and inside the forced regime a point count that is no multiple of 4 or above 2048:
    PIT_ERR_UNSUPPORTED before any launch, nothing written."""
    L = _lib_()
    assert L.lib().pit_posatt_pre_supported(770, 2, 256, 4) == 0 and L.lib().pit_posatt_pre_supported(100, 2, 64, 4) == 0
    p = Pre(100, 4, 64, 2, seed=2)                # outside the regime (unforced)
    p.forward({}, rc_want=UNSUPPORTED)
    p.backward({}, rc_want=UNSUPPORTED)
    monkeypatch.setenv("PIT_FORCE_TILES", "1")
    p = Pre(102, 4, 64, 2, seed=2)                # 102 % 4 != 0
    p.forward({}, rc_want=UNSUPPORTED)
    p.backward({}, rc_want=UNSUPPORTED)
    assert L.lib().pit_posatt_pre_supported(2048, 1, 64, 4) == 1 and L.lib().pit_posatt_pre_supported(2052, 1, 64, 4) == 0
    p = Pre(2052, 4, 64, 1, seed=2)               # more than 2048 points
    p.forward({}, rc_want=UNSUPPORTED)
    p.backward({}, rc_want=UNSUPPORTED)


# --------------------------------------------------------------------------- 4..8 coordinates
WIDE = [
    _case("wide-sdim4-w1", 45, 40, 2, 48, 2, sdim=4, w_rows=1, w_cols=2, grid_r=(3, 2, 2), grid_c=(3, 2, 1)),
    _case("wide-sdim5-w8-masked", 130, 257, 2, 70, 2, sdim=5, loc=0.3, w_rows=8, w_cols=8, grid_r=(5, 2, 5), grid_c=(5, 9, 1)),
    _case("wide-sdim8-w8-per-sample", 130, 300, 3, 33, 1, sdim=8, per_sample=True, w_rows=8, w_cols=4, grid_r=(6, 1, 5), grid_c=(2, 10, 3)),
    _case("wide-sdim8-w1-masked", 33, 50, 2, 48, 1, sdim=8, loc=0.3, w_rows=1, w_cols=1, grid_r=(3, 1, 2), grid_c=(3, 2, 1)),
]


@pytest.mark.parametrize("c", WIDE)
def test_meshes_of_4_to_8_coordinates(c):
    """posatt_rows_kernel8 (forward fp32 / bf16, d(scale)) and posatt_cols_kernel8 at 1 and 8 waves; the pair declines (two launches)."""
    r = Run(c)
    rows, cols = dict(rows8=c["w_rows"], grid=c["grid_r"]), dict(cols8=c["w_cols"], grid=c["grid_c"])
    r.forward(rows)
    r.forward(rows, mode=BF16)
    r.backward(rows, False, True)
    r.backward(cols, True, False)
    r.backward(cols, True, False, mode=BF16)
    r.backward(dict(rows8=c["w_rows"], cols8=c["w_cols"], grid=c["grid_c"]), True, True)


# --------------------------------------------------------------------------- periodic metrics
METRICS = [
    _case("metric-periodic1d-jsplit", 70, 100, 2, 48, 2, metric="periodic1d", loc=0.1, cmul=40.0, tiles=False,
          rows=dict(rows=(1, 2, 0), grid=(3, 2, 3)), cols=dict(cols=(1, 4, 0), grid=(3, 4, 1))),
    _case("metric-periodic2d-jsplit", 70, 144, 2, 48, 2, metric="periodic2d", loc=0.1, cmul=10.0, tiles=False,
          rows=dict(rows=(1, 4, 0), grid=(3, 2, 3)), cols=dict(cols=(1, 4, 0), grid=(3, 5, 1))),
    _case("metric-periodic1d-tiles", 100, 257, 4, 64, 2, metric="periodic1d", loc=0.1, cmul=40.0, tiles=True,
          rows=dict(trows=(1, 8), grid=(1, 2, 4)), cols=dict(tcols=8, grid=(1, 9, 1))),
    _case("metric-periodic2d-tiles", 100, 289, 4, 64, 2, metric="periodic2d", loc=0.1, cmul=10.0, tiles=True,
          rows=dict(trows=(1, 8), grid=(1, 2, 4)), cols=dict(tcols=8, grid=(1, 10, 1))),
]


@pytest.mark.parametrize("c", METRICS)
def test_periodic_metrics(c, monkeypatch):
    """The PER variant of the step, masked, with rows whose nearest keys lie across the wrap (asserted on the reference)."""
    if c["tiles"]:
        monkeypatch.setenv("PIT_FORCE_TILES", "1")
        monkeypatch.setenv("PIT_FORCE_RT", "1")
    r = Run(c)
    r.forward(c["rows"])
    r.backward(c["rows"], False, True)
    r.backward(c["cols"], True, False)


# --------------------------------------------------------------------------- call forms and flags
def test_concat_form_and_residual():
    """copy_inputs (masked self attention into a concat buffer, out_col0 = dim) and add_residual in the backward, alone and merged."""
    r = Run(dict(n_out=70, n_in=70, batch=2, dim=48, heads=2, loc=0.3, self_attn=True, col0=48))
    r.forward(dict(rows=(1, 2, 0), grid=(3, 2, 3)), copy=True)
    r.backward(dict(cols=(1, 4, 0), grid=(3, 3, 1)), True, False, resid=True)
    r.backward(dict(pair=(1, 2, 0), grid=(27, 1, 1)), True, True, resid=True)
    r.backward(dict(pair=(1, 2, 0), grid=(27, 1, 1)), True, True, resid=True, mode=BF16)


def test_unmasked_self_attention_without_statistics():
    """stats == NULL: S_min = 0 in the kernel and in the reference."""
    r = Run(dict(n_out=70, n_in=70, batch=2, dim=48, heads=2, self_attn=True))
    assert r.stats is None
    r.forward(dict(rows=(1, 2, 0), grid=(3, 2, 3)))
    r.backward(dict(pair=(1, 2, 0), grid=(27, 1, 1)), True, True)


def test_out_col0_without_concat():
    r = Run(dict(n_out=70, n_in=100, batch=2, dim=48, heads=2, col0=3, loc=0.3))
    r.forward(dict(rows=(1, 2, 0), grid=(3, 2, 3)))
    r.backward(dict(pair=(1, 2, 0), grid=(30, 1, 1)), True, True)


def _ulps(a, b):
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


def test_head_handed_over_as_lmda():
    """head_is_scale = 0: scale_out within 24 ulp of the oracle's head_scale (tests/test_gpu_ops.py)."""
    r = Run(dict(n_out=70, n_in=100, batch=2, dim=48, heads=2))
    lmda = torch.tensor([0.3, -0.7])
    so = r.forward(dict(rows=(1, 2, 0), grid=(3, 2, 3)), lmda=lmda)
    assert _ulps(so.cpu().view(-1), orc.head_scale(lmda)) <= 24


def test_accumulated_and_deferred_head_gradient():
    """PIT_HEAD_ACCUMULATE onto a non-zero d_head; PIT_HEAD_DEFER leaves the slots loaded and d_head alone until
    pit_posatt_dhead_finish drains them."""
    r = Run(dict(n_out=70, n_in=100, batch=2, dim=48, heads=3))
    d0 = r.ref["r64"]["dc"].float() * torch.tensor([0.5, -2.0, 1.0])
    r.backward(dict(rows=(1, 2, 0), grid=(3, 3, 3)), False, True, acc=HEAD_ACCUMULATE, dhead0=d0)
    work, dhead = r.backward(dict(pair=(1, 2, 0), grid=(39, 1, 1)), True, True, acc=HEAD_DEFER)
    assert float(work.abs().max()) > 0.0 and dhead.unwritten()
    L = _lib_()
    arr = lambda v: (ctypes.c_void_p * 1)(v)
    rc = L.lib().pit_posatt_dhead_finish(1, arr(work.data_ptr()), arr(dhead.ptr), arr(r.head.ptr), arr(r.head.ptr),
                                         (ctypes.c_int * 1)(3), (ctypes.c_int * 1)(HEAD_IS_SCALE), None, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and float(work.abs().max()) == 0.0 and dhead.untouched()
    compare("d(c)[deferred]", dhead.cpu(), r.ref["r64"]["dc"].reshape(1, 1, -1), TOL["dc"], 1, 1)


def test_argument_refusals_write_nothing():
    """copy_inputs / add_residual with n_out != n_in (PIT_ERR_SIZE), NULL statistics on a masked call (PIT_ERR_NULL), bf16 out /
    d_out storage on a dense call (PIT_ERR_UNSUPPORTED): before any launch."""
    r = Run(dict(n_out=70, n_in=100, batch=2, dim=48, heads=2, loc=0.3, col0=48))
    r.forward({}, copy=True, rc_want=ERR_SIZE)
    r.forward({}, stats=False, rc_want=ERR_NULL)
    r.forward({}, mode=BF16 | OUT16, rc_want=UNSUPPORTED)
    r.backward({}, True, True, resid=True, rc_want=ERR_SIZE)
    r.backward({}, True, True, mode=BF16 | DOUT16, rc_want=UNSUPPORTED)
    r = Run(dict(n_out=70, n_in=100, batch=2, dim=48, heads=2))       # unmasked cross attention needs the row minimum as well
    r.forward({}, stats=False, rc_want=ERR_NULL)


# --------------------------------------------------------------------------- PIT_NO_FAST_LOADS
def test_checked_loads_everywhere(monkeypatch):
    """PIT_NO_FAST_LOADS=1 (read per call): the range-checked loads in the steady state of a J-split rows launch, a tiles rows
    launch and a precomputed-weights launch, held to the bounds of their fast twins."""
    monkeypatch.setenv("PIT_NO_FAST_LOADS", "1")
    c = dict(n_out=64, n_in=257, batch=2, dim=48, heads=1, loc=0.2)
    r = Run(c)
    r.forward(dict(rows=(1, 8, 0), grid=(3, 1, 2)))
    r.forward(dict(rows=(1, 8, 0), grid=(3, 1, 2)), mode=BF16)
    r.backward(dict(pair=(1, 2, 0), grid=(6 + 27, 1, 1)), True, True)
    monkeypatch.setenv("PIT_FORCE_TILES", "1")
    monkeypatch.setenv("PIT_FORCE_RT", "2")
    r = Run(dict(n_out=100, n_in=129, batch=4, dim=64, heads=2))
    r.forward(dict(trows=(2, 8), grid=(1, 2, 2)))
    r.backward(dict(trows=(2, 8), tcols=8, grid=(1, 5, 1)), True, True)
    p = Pre(100, 4, 64, 1, seed=2)
    p.forward(dict(trows=(2, 8), grid=(1, 1, 2)))
    p.backward(dict(tcols=8, trows=(2, 8), grid=(1, 1, 2)))


# --------------------------------------------------------------------------- exact ties at the threshold
DUP = [
    _case("dup-jsplit", 70, 100, 2, 48, 2, loc=0.12, dup=(20, 3), tiles=False,
          rows=dict(rows=(1, 2, 0), grid=(3, 2, 3)), pair=dict(pair=(1, 2, 0), grid=(30, 1, 1))),
    _case("dup-tiles", 100, 257, 4, 64, 2, loc=0.05, dup=(20, 3), tiles=True,
          rows=dict(trows=(1, 8), grid=(1, 2, 4)), pair=dict(trows=(1, 8), tcols=8, grid=(1, 9, 1))),
]


@pytest.mark.parametrize("c", DUP)
def test_duplicated_keys_tie_at_the_threshold(c, monkeypatch):
    """20 copies of one key and 3 rows sitting on them: m_(k) == m_(k+1) for the rows whose k-th neighbour is a copy, so their
    score EQUALS the threshold (asserted on the reference) and all copies are kept."""
    if c["tiles"]:
        monkeypatch.setenv("PIT_FORCE_TILES", "1")
        monkeypatch.setenv("PIT_FORCE_RT", "1")
    r = Run(c)
    r.forward(c["rows"])
    r.backward(c["pair"], True, True)


# --------------------------------------------------------------------------- the record itself
def test_record_is_per_thread_and_resets():
    from position_induced_transformer_amd import ops
    r = Run(dict(n_out=70, n_in=33, batch=2, dim=48, heads=1))
    L = _lib_()
    out, rowstat = Buf(2, 70, 48), Buf(1, 70, 4)
    call = lambda: L.lib().pit_posatt_fwd(*r._mesh(), r.V.ptr, 2, 48, r.V.ld, r.V.bs, r.head.ptr, 1, 1, r.stats.ptr, 0.0, 0, 0,
                                          out.ptr, out.ld, out.bs, 0, 0, rowstat.ptr, None, None, None, 0, 0, 0, L.stream_ptr())
    dense_counts()
    assert call() == 0 and call() == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.dense_launch_counts(reset=True)))
    t.start()
    t.join()
    assert not any(seen[0]), "another thread sees this thread's launches"
    want = dict(rows_fwd=2, last_rows=11000, grid_x=3, grid_y=1, grid_z=3)
    assert dense_counts(reset=False) == want                                   # ... and did not reset them
    assert dense_counts() == want and dense_counts() == {}
    torch.cuda.synchronize()
