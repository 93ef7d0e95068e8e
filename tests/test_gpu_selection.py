"""csrc/pit_select.hip - row order statistics, candidate lists, transposed lists - at every instance its four host dispatchers
can choose, against torch.sort on the CPU.  Everything here is exact: statistics as bit patterns, lists as integer sets; no
tolerance appears in this module.  The C entries are called directly (``_lib.lib()``), so cap, rank_k, flags and the reverse-list
pointers are free.  Every output buffer is handed over DIRTY (the entries clear what they need themselves).

The reference (CPU, fp32):
* distances as oracle/pit_oracle.py forms them (sqdist_euclid / _periodic1d / _periodic2d, the period passed in as the entries
  take it; the CPU test at the end pins ``sqdist`` here to the oracle's own functions bit for bit);
* ``srt = torch.sort(m)``: the statistics are srt[k], srt[min(k + 1, J - 1)], srt[0];
* the candidate set of a row is EXACTLY { j : m_j <= fl32(m_(k+1) * fl32(1 + 2^-21)) } (one IEEE fp32 multiply), nbr_cnt its size
  (also beyond cap); the wave-per-row and two-pass kernels write it in ascending key order, truncated to cap (the array prefix
  is compared); the lane kernel orders by block (sorted rows are compared; of a row with cnt > cap only that its cap entries
  are distinct members);
* transposed lists: a CPU transposition of the device's own nbr_idx / nbr_cnt, which the same test has just checked
  (``check_transpose``).

How a case maps to a kernel instance (the dispatch rules of select_fwd / pit_plan_fwd, re-computed and asserted):
* pit_select_fwd: select_rows_reg<ITEMS>, ITEMS = first of {1, 2, 4, 8, 16, 32, 64} >= ceil(n_in / 64); select_rows_stream
  beyond 4096 keys; select_rows_stream8 for 4..8 coordinates (pit_select_wide_fwd).
* pit_plan_fwd, wave per row: plan_rows_reg<ITEMS>, ITEMS = first of {1, 2, 4, 8, 12, 16, 24, 32, 64} >= ceil(n_in / 64); beyond
  4096 keys or with PIT_PLAN_TWO_PASSES: select_fwd + neighbors_kernel.  Inside plan_row_wave the search is narrowed when
  ITEMS >= 4 and k + 2 <= 32 and at most 64 keys are <= U, U the (k+2)-th smallest of the 64 lane minima (``narrow_total``
  recomputes that count on the CPU; the cases sit on 64, above 64, and on k + 2 = 32 / 33).  (Its fourth condition, U =
  0xFFFFFFFF, needs fewer than k + 2 lanes with a key: impossible at ITEMS >= 4, i.e. n_in >= 129 >= 64 - not reachable.)
* pit_plan_fwd, lane per row (plan_rows_lane<SD2, PER, 64, 6>): mesh_batch > 1, rank_k + 2 <= 64, n_in <= 4096, rows >= 32768,
  no PIT_PLAN_WAVE_PER_ROW, and lane_sm = ceil64(n_in) * (SD2 ? 8 : 16) + 20480 + (rev ? 4 n_in : 0) <= 65536 bytes.  That limit
  is n_in 3712 | 3713 for a 2-coordinate mesh with reverse lists (29696 + 20480 + 14848 = 65024; 30208 + 20480 + 14852 = 65540)
  and 2816 | 2817 for a 3-coordinate mesh without (45056 + 20480 = 65536; 46080 + 20480).  Without reverse lists a 2-coordinate
  mesh never reaches it (4096 keys: 53248 bytes).  Flagged rows go to plan_rows_fix<4 | 16 | 64> by ceil(n_in / 64) <= 4 | <= 16.
  Which kernel ran is visible in the output: the wave kernels write every list ascending, the lane kernel by block (key j
  belongs to block j % 64), so some list is not ascending.
* transposed lists: nbr_count_lds / nbr_scan_kernel / nbr_fill_lds up to 4096 keys (128 rows per workgroup, 256 keys per scan
  chunk), beyond: counts from neighbors_kernel's own atomics + nbr_fill_kernel.

Not reachable through the entries: the NB = 32 instances of plan_rows_lane (the dispatcher fixes nb = 64); plan_rows_reg with
its own count atomics (needs n_in > 4096, which takes the two passes).  At rank_k >= 39 a list holds k + 2 > 40 keys, more than a
lane's column: the lane kernel then flags every row and plan_rows_fix writes every list, so at the rank_k 62 | 63 edge both sides
are compared with the sort and with each other, but the output cannot show which kernel ran (the same when all keys coincide).

Conditions on the reference alone, asserted in every case: a case meant not to overflow has count <= cap on every row; a case
meant to overflow has a row over cap and a row at or under it (cap = 1 excepted: a list has at least k + 2 >= 2 entries, so
with cap = 1 every row overflows - asserted as such).
"""
import functools

import pytest
import torch

import pit_oracle as orc

gpu = pytest.mark.gpu

EUC, P1, P2 = 0, 1, 2                                   # PIT_METRIC_*
WAVE_PER_ROW, TWO_PASSES = 1, 2                         # PIT_PLAN_*
ERR_UNSUPPORTED = -4
ONE_P21 = torch.tensor(1.0 + 2.0 ** -21, dtype=torch.float32)
BIG = torch.iinfo(torch.int32).max

# (name, metric, space_dim)
FORMS = {"euc1": (EUC, 1), "euc2": (EUC, 2), "euc3": (EUC, 3), "per1": (P1, 1), "per2": (P2, 2), "per3": (P2, 3),
         "per1of2": (P1, 2), "euc5": (EUC, 5), "euc8": (EUC, 8), "per5": (P2, 5)}
KINDS = ("cloud", "dups", "same", "hits", "grid")
GROUPS = (3, 20, 7, 45, 100)                            # duplicated key points (sizes taken while they fill < 70 % of the keys)


# --------------------------------------------------------------------------- reference
def sqdist(metric, mo, mi, period):
    """(b, N, s) x (b, J, s) -> (b, N, J) fp32, the operations of pit_oracle.sqdist_* in their order."""
    if metric == EUC:
        return orc.sqdist_euclid(mo, mi)
    d = abs(mo.unsqueeze(-2) - mi.unsqueeze(-3))
    d = torch.minimum(d, torch.tensor(period, dtype=torch.float32) - d)
    return d[..., 0] ** 2 if metric == P1 else torch.sum(d ** 2, dim=-1)


def ref_rows(m, k):
    """m (R, J) -> stats (3, R), member (R, J) bool, count (R)."""
    J = m.shape[1]
    srt = torch.sort(m, dim=1).values
    st = torch.stack([srt[:, k], srt[:, min(k + 1, J - 1)], srt[:, 0]])
    member = m <= (st[1] * ONE_P21)[:, None]
    return st, member, member.sum(1).to(torch.int32)


def expected_prefix(member, cap):
    """The set in ascending key order, truncated to cap, -1 beyond."""
    rank = member.long().cumsum(1) - 1
    r, j = (member & (rank < cap)).nonzero(as_tuple=True)
    out = torch.full((member.shape[0], cap), -1, dtype=torch.int32)
    out[r, rank[r, j]] = j.to(torch.int32)
    return out


def narrow_total(m, k):
    """Keys at or below U, the (k+2)-th smallest of the 64 lane minima (key j sits in lane j % 64): plan_row_wave's `total`."""
    R, J = m.shape
    pad = torch.full((R, (J + 63) // 64 * 64), float("inf"))
    pad[:, :J] = m
    lmin = pad.view(R, -1, 64).min(1).values
    U = lmin.sort(1).values[:, k + 1]
    return (m <= U[:, None]).sum(1)


def bits(x):
    return x.contiguous().view(torch.int32)


def plan_items(n_in):
    return next(v for v in (1, 2, 4, 8, 12, 16, 24, 32, 64, 1 << 30) if (n_in + 63) // 64 <= v)


def lane_expected(b, n_out, n_in, coords, k, rev, flags):
    """pit_plan_fwd's lane_ok && lane_sm <= 65536."""
    sm = (n_in + 63) // 64 * 64 * (2 if coords <= 2 else 4) * 4 + 40 * 256 * 2 + (4 * n_in if rev else 0)
    return (b > 1 and k + 2 <= 64 and n_in <= 4096 and b * n_out >= 32768 and not (flags & (WAVE_PER_ROW | TWO_PASSES))
            and coords <= 3 and sm <= 65536)


# --------------------------------------------------------------------------- meshes
def make_mesh(kind, b, n_out, n_in, sd, seed, groups=GROUPS, near_every=4):
    """Meshes in [0, 1)^sd (period 1 for the periodic metrics).  Returns mo, mi and near (n_out,): the size of the duplicate
    group row r was put next to, 0 for none."""
    g = torch.Generator().manual_seed(seed)
    mo, mi = torch.rand(b, n_out, sd, generator=g), torch.rand(b, n_in, sd, generator=g)
    near = torch.zeros(n_out, dtype=torch.long)
    if kind == "dups":
        sizes, used = [], 0
        for s in groups:
            if used + s <= 0.7 * n_in:
                sizes.append(s)
                used += s
        assert sizes, (n_in, groups)
        for smp in range(b):
            perm = torch.randperm(n_in, generator=g)            # members scattered over the lanes / blocks
            loc = 0.1 + 0.8 * torch.rand(len(sizes), sd, generator=g)
            o = 0
            for gi, s in enumerate(sizes):
                mi[smp, perm[o:o + s]] = loc[gi]
                o += s
            r = torch.arange(1, n_out, near_every)              # every near_every-th row sits next to a group
            gi = (r // near_every) % len(sizes)
            mo[smp, r] = loc[gi] + 1e-3 * (torch.rand(len(r), sd, generator=g) - 0.5)
            near[r] = torch.tensor(sizes)[gi]
    elif kind == "same":
        mi[:] = mi[:, :1]
    elif kind == "hits":
        r = torch.arange(0, n_out, 2)
        mo[:, r] = mi[:, (r * 7) % n_in]
    elif kind == "grid":
        side = 1
        while side ** sd < n_in:
            side *= 2                                           # power of two: node coordinates are exact, tie shells are exact ties
        j = torch.arange(n_in)
        mi = torch.stack([(j // side ** c) % side for c in range(sd)], -1).float().div(side)[None].repeat(b, 1, 1).contiguous()
        r = (torch.arange(n_out) * 13) % n_in
        mo = mi[:, r] + (torch.arange(n_out) % 2).float()[None, :, None] * (0.5 / side)      # on nodes and on cell centres
    elif kind == "tiny":                                        # squared distances around 2^-133: subnormal floats (and their products with 1 + 2^-21)
        mo, mi = mo * 2.0 ** -66, mi * 2.0 ** -66
    else:
        assert kind == "cloud", kind
    return mo.contiguous(), mi.contiguous(), near


class Case:
    """Meshes + the reference of the rows asked for (all rows by default), computed once."""
    def __init__(self, kind, form, b, n_out, n_in, seed, **kw):
        self.metric, self.sd = FORMS[form]
        self.coords = 1 if self.metric == P1 else self.sd
        self.period = 1.0
        self.b, self.n_out, self.n_in = b, n_out, n_in
        self.mo, self.mi, self.near = make_mesh(kind, b, n_out, n_in, self.sd, seed, **kw)
        self.id = f"{kind}-{form}-b{b}-N{n_out}-J{n_in}"
        self._m = {}

    def m(self, rows=None):
        """(b, R, J) distances of the rows (a LongTensor of row indices inside a sample, or all)."""
        key = None if rows is None else tuple(rows.tolist())
        if key not in self._m:
            mo = self.mo if rows is None else self.mo[:, rows]
            self._m = {key: sqdist(self.metric, mo, self.mi, self.period)}
        return self._m[key]

    def ref(self, k, rows=None):
        m = self.m(rows)
        out = [ref_rows(m[s], k) for s in range(self.b)]
        return (torch.stack([o[0] for o in out], 1), torch.stack([o[1] for o in out]), torch.stack([o[2] for o in out]))


def cap_for(count, want):
    """want 'fit': the largest reference count (some row sits exactly on cap); an int: an overflow case."""
    if want == "fit":
        return int(count.max())
    return want


def assert_reference_conditions(count, cap, want, what):
    if want == "fit":
        assert int(count.max()) <= cap, what
    elif cap == 1:
        assert int(count.min()) > 1, what                       # (k + 2 >= 2 entries on every list)
    else:
        assert int(count.max()) > cap and int(count.min()) <= cap, (what, int(count.min()), int(count.max()))


# --------------------------------------------------------------------------- device calls
def dev_select(c, k, need_kth, wide=False):
    from position_induced_transformer_amd import _lib
    mo, mi = c.mo.cuda(), c.mi.cuda()
    stats = torch.full((3, c.b, c.n_out), float("nan"), device="cuda")
    fn = _lib.lib().pit_select_wide_fwd if wide else _lib.lib().pit_select_fwd
    rc = fn(mo.data_ptr(), mi.data_ptr(), c.b, c.n_out, c.n_in, c.sd, c.metric, c.period, k, need_kth, stats.data_ptr(),
            _lib.stream_ptr())
    assert rc == 0, (c.id, k, rc)
    torch.cuda.synchronize()
    return stats.cpu()


def plan_buffers(c, cap, rev):
    d = dict(stats=torch.full((3, c.b, c.n_out), float("nan"), device="cuda"),
             idx=torch.full((c.b, c.n_out, cap), -7, dtype=torch.int32, device="cuda"),
             cnt=torch.full((c.b, c.n_out), -9, dtype=torch.int32, device="cuda"))
    if rev:
        d.update(rev_ptr=torch.full((c.b, c.n_in + 1), 0x5a5a5a, dtype=torch.int32, device="cuda"),
                 rev_row=torch.full((c.b, c.n_out * cap), 123456789, dtype=torch.int32, device="cuda"),
                 ws=torch.full((2 * c.b * c.n_in,), 0x3c3c3c, dtype=torch.int32, device="cuda"))
    return d


def dev_plan(c, k, cap, rev, flags, bufs=None, to_cpu=True):
    from position_induced_transformer_amd import _lib
    mo, mi = c.mo.cuda(), c.mi.cuda()
    d = bufs or plan_buffers(c, cap, rev)
    p = lambda n: d[n].data_ptr() if n in d else 0
    rc = _lib.lib().pit_plan_fwd(mo.data_ptr(), mi.data_ptr(), c.b, c.n_out, c.n_in, c.sd, c.metric, c.period, k,
                                 p("stats"), cap, p("idx"), p("cnt"), p("rev_ptr"), p("rev_row"), p("ws"), flags,
                                 _lib.stream_ptr())
    assert rc == 0, (c.id, k, cap, rev, flags, rc)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in d.items() if n != "ws"} if to_cpu else d


def dev_neighbors(c, stats, cap, rev):
    """pit_neighbors_fwd on the statistics given (a CPU tensor (3, b, n_out))."""
    from position_induced_transformer_amd import _lib
    mo, mi = c.mo.cuda(), c.mi.cuda()
    d = plan_buffers(c, cap, rev)
    d["stats"] = stats.cuda().contiguous()
    p = lambda n: d[n].data_ptr() if n in d else 0
    rc = _lib.lib().pit_neighbors_fwd(mo.data_ptr(), mi.data_ptr(), c.b, c.n_out, c.n_in, c.sd, c.metric, c.period, p("stats"), cap,
                                      p("idx"), p("cnt"), p("rev_ptr"), p("rev_row"), p("ws"), _lib.stream_ptr())
    assert rc == 0, (c.id, cap, rev, rc)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in d.items() if n != "ws"}


def dev_transpose(c, idx, cnt, cap, bufs=None):
    from position_induced_transformer_amd import _lib
    d = bufs or {n: v for n, v in plan_buffers(c, cap, True).items() if n in ("rev_ptr", "rev_row", "ws")}
    i, n = idx.cuda().contiguous(), cnt.cuda().contiguous()
    rc = _lib.lib().pit_lists_transpose(i.data_ptr(), n.data_ptr(), c.b, c.n_out, c.n_in, cap, d["rev_ptr"].data_ptr(),
                                        d["rev_row"].data_ptr(), d["ws"].data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, d


# --------------------------------------------------------------------------- comparisons
def masked(idx, cnt, cap, fill=-1):
    """(.., cap) lists with the slots from min(cnt, cap) on replaced."""
    col = torch.arange(cap, device=idx.device) < torch.clamp(cnt, max=cap).unsqueeze(-1)
    return torch.where(col, idx, torch.full_like(idx, fill))


def all_ascending(idx, cnt, cap):
    a = masked(idx, cnt, cap, BIG).long()
    return bool((a[..., 1:] >= a[..., :-1]).all())


def check_stats(got, want, what):
    for i, name in enumerate(("m_(k)", "m_(k+1)", "m_min")):
        bad = (bits(got[i]) != bits(want[i])).nonzero()
        assert bad.numel() == 0, (what, name, bad[:4].tolist(), got[i][tuple(bad[0])].item(), want[i][tuple(bad[0])].item())


def check_lists_ordered(out, member, count, cap, what):
    """wave-per-row / two-pass kernels: true counts, the exact array prefix."""
    bad = (out["cnt"] != count).nonzero()
    assert bad.numel() == 0, (what, "nbr_cnt", bad[:4].tolist(), out["cnt"][tuple(bad[0])].item(), count[tuple(bad[0])].item())
    want = torch.stack([expected_prefix(member[s], cap) for s in range(member.shape[0])])
    got = masked(out["idx"], out["cnt"], cap)
    bad = (got != want).any(-1).nonzero()
    assert bad.numel() == 0, (what, "nbr_idx", bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def check_lists_as_sets(idx, cnt, member, count, cap, what):
    """lane kernel: true counts; rows within cap as sorted sets; rows beyond cap: cap distinct members."""
    assert torch.equal(cnt, count), (what, "nbr_cnt", (cnt != count).nonzero()[:4].tolist())
    got = masked(idx, cnt, cap, BIG).sort(-1).values
    want = torch.stack([expected_prefix(member[s], cap) for s in range(member.shape[0])])
    want = torch.where(want < 0, torch.full_like(want, BIG), want)
    fits = count <= cap
    bad = ((got != want).any(-1) & fits).nonzero()
    assert bad.numel() == 0, (what, "nbr_idx", bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    over = (~fits).nonzero()
    if over.numel():
        g = got[over[:, 0], over[:, 1]].long()                   # (n_over, cap), all cap slots written
        assert bool((g[:, 1:] > g[:, :-1]).all()) and bool((g >= 0).all()) and bool((g < member.shape[-1]).all()), (what, "distinct")
        assert bool(member[over[:, 0], over[:, 1]].gather(1, g).all()), (what, "members")


def check_transpose(idx, cnt, cap, rev_ptr, rev_row, n_in, what):
    """rev_ptr / rev_row against a CPU transposition of (idx, cnt): see the module docstring."""
    b, n_out = cnt.shape
    for s in range(b):
        slot = torch.arange(cap)[None, :] < torch.clamp(cnt[s], max=cap)[:, None]
        keys = idx[s][slot].long()
        assert bool(((keys >= 0) & (keys < n_in)).all()), what
        count_all = torch.bincount(keys, minlength=n_in)
        p = rev_ptr[s].long()
        assert int(p[0]) == 0, (what, s)
        bad = ((p[1:] - p[:-1]) != count_all).nonzero()
        assert bad.numel() == 0, (what, s, "rev_ptr", bad[:4].tolist())
        total = int(p[n_in])
        assert bool((rev_row[s][total:] == -1).all()), (what, s, "beyond rev_ptr[n_in]")
        fill = slot & (cnt[s] <= cap)[:, None]
        rows = torch.arange(n_out)[:, None].expand(-1, cap)[fill]
        want = (idx[s][fill].long() * n_out + rows).sort().values
        keyid = torch.repeat_interleave(torch.arange(n_in), count_all)
        got = rev_row[s][:total].long()
        pos = got >= 0
        assert bool((got[~pos] == -1).all()) and bool((got[pos] < n_out).all()), (what, s, "entries")
        gotp = (keyid[pos] * n_out + got[pos]).sort().values
        assert gotp.shape == want.shape and torch.equal(gotp, want), (what, s, "rev_row", gotp.numel(), want.numel())


# =========================================================================== 1. pit_select_fwd
SELECT_N = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)
SELECT_FORMS = ("euc1", "euc2", "euc3", "per1", "per2")


def ranks(n_in):
    return sorted({0, min(1, n_in - 1), max(n_in - 2, 0), n_in - 1, n_in // 3})


@gpu
@pytest.mark.parametrize("form", SELECT_FORMS)
@pytest.mark.parametrize("n_in", SELECT_N)
def test_select_fwd_statistics_equal_the_sort_bit_for_bit(n_in, form):
    """select_rows_reg<1..64> on both sides of every ITEMS edge and select_rows_stream at 4097: ranks 0, 1, a middle one, n_in - 2
    and n_in - 1 (k + 1 clipped), need_kth 0 and 1; 2 samples x 7 rows (the second workgroup straddles the samples, the last one
    has idle waves)."""
    i = SELECT_N.index(n_in) + SELECT_FORMS.index(form)
    for kind in (KINDS[i % 5], KINDS[(i + 2) % 5], "tiny"):
        if kind == "dups" and n_in < 8:
            kind = "same"
        c = Case(kind, form, 2, 7, n_in, seed=100 + i)
        for k in ranks(n_in):
            want, _, _ = c.ref(k)
            check_stats(dev_select(c, k, 1), want, (c.id, k))
        got = dev_select(c, 0, 0)                                # need_kth = 0: the row minimum (stats[2]) is what is promised
        assert torch.equal(bits(got[2]), bits(c.ref(0)[0][2])), c.id


@gpu
@pytest.mark.parametrize("form", ["euc5", "euc8", "per5"])
@pytest.mark.parametrize("n_in", [100, 4200])
def test_select_wide_fwd_statistics_equal_the_sort_bit_for_bit(n_in, form):
    """select_rows_stream8 (5 and 8 coordinates) at a short row and beyond 4096 keys."""
    for kind in KINDS:
        c = Case(kind, form, 2, 5, n_in, seed=7 + n_in)
        for k in (0, n_in // 3, n_in - 1):
            check_stats(dev_select(c, k, 1, wide=True), c.ref(k)[0], (c.id, k))
        assert torch.equal(bits(dev_select(c, 0, 0, wide=True)[2]), bits(c.ref(0)[0][2])), c.id


# =========================================================================== 2. pit_plan_fwd, a wavefront per row
WAVE_N = (64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 4096, 4097)
WAVE_FORMS = ("euc2", "euc3", "per2", "euc1", "per1", "per3", "per1of2")


def wave_configs(n_in):
    """(kind, form, rank_k, cap wanted).  Every n_in: ranks 30 / 31 (k + 2 = 32 / 33: the narrowed search's rank edge wherever
    ITEMS >= 4), caps 1 / 4 / 16 with overflowing and fitting rows, a clipped k + 1, every mesh kind."""
    i = WAVE_N.index(n_in)
    f = lambda o: WAVE_FORMS[(i + o) % len(WAVE_FORMS)]
    return [("cloud", f(0), 30, "fit"), ("cloud", f(0), 31, "fit"),
            ("dups", f(1), 2, 4), ("dups", f(2), 14, 16), ("dups", f(3), 5, "fit"),
            ("hits", f(4), 0, 1), ("hits", f(4), 3, "fit"),
            ("same", f(5), 1, "fit"), ("tiny", f(3), 7, "fit"),
            ("grid", f(6), n_in // 5, "fit"), ("grid", f(1), n_in - 1, "fit"), ("grid", f(2), n_in - 2, "fit")]


def run_wave_case(c, k, want_cap, what):
    """One-pass and two-pass plan, with and without reverse lists: all equal to the reference and to each other."""
    want, member, count = c.ref(k)
    cap = cap_for(count, want_cap)
    assert_reference_conditions(count, cap, want_cap, what)
    assert not lane_expected(c.b, c.n_out, c.n_in, c.coords, k, True, 0)
    outs = {}
    for flags in (0, TWO_PASSES):
        for rev in (False, True):
            o = outs[flags, rev] = dev_plan(c, k, cap, rev, flags)
            w = (what, "flags", flags, "rev", rev)
            check_stats(o["stats"], want, w)
            check_lists_ordered(o, member, count, cap, w)
            if rev:
                check_transpose(o["idx"], o["cnt"], cap, o["rev_ptr"], o["rev_row"], c.n_in, w)
    a, t = outs[0, True], outs[TWO_PASSES, True]
    assert torch.equal(bits(a["stats"]), bits(t["stats"])) and torch.equal(a["cnt"], t["cnt"])
    assert torch.equal(masked(a["idx"], a["cnt"], cap), masked(t["idx"], t["cnt"], cap)) and torch.equal(a["rev_ptr"], t["rev_ptr"])
    return outs, cap


@gpu
@pytest.mark.parametrize("n_in", WAVE_N)
def test_wave_per_row_plan_equals_the_sort_and_the_two_pass_plan(n_in):
    """plan_rows_reg<1..64> on both sides of every ITEMS edge, 4097 keys on the two streaming passes; 2 samples x 37 rows."""
    assert plan_items(n_in) == {64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8, 513: 12, 768: 12, 769: 16, 1024: 16, 1025: 24,
                                1536: 24, 1537: 32, 2048: 32, 2049: 64, 4096: 64, 4097: 1 << 30}[n_in]
    fitted = {}
    for n, (kind, form, k, want_cap) in enumerate(wave_configs(n_in)):
        c = Case(kind, form, 2, 37, n_in, seed=1000 + 17 * WAVE_N.index(n_in) + n)
        run_wave_case(c, k, want_cap, (c.id, "k", k, "cap", want_cap))
        if kind == "cloud":
            fitted[k] = bool((narrow_total(c.m()[0], k) <= 64).any())
    if 4 <= plan_items(n_in) <= 64:                              # k + 2 = 32 narrows on some row of a random cloud (33 never does)
        assert fitted[30], n_in


@gpu
@pytest.mark.parametrize("n_in", [300, 1100, 4000])
@pytest.mark.parametrize("group", [64, 65, 100])
def test_wave_per_row_plan_at_the_64_candidate_edge_of_the_narrowed_search(n_in, group):
    """Rows next to `group` identical keys, rank 5: exactly 64 keys at or below the bound U (the narrowed search still fits one
    candidate per lane), 65 and 100 (it does not: the full search)."""
    c = Case("dups", "euc2", 2, 37, n_in, seed=50 + n_in + group, groups=(group,), near_every=2)
    tot = torch.cat([narrow_total(c.m()[s], 5) for s in range(c.b)])
    assert bool((tot == group).any()) and bool((tot < 64).any()), (c.id, tot.tolist())
    run_wave_case(c, 5, "fit", (c.id, "k", 5))
    run_wave_case(c, 5, 16, (c.id, "k", 5, "cap", 16))


@gpu
@pytest.mark.parametrize("form", ["euc5", "euc8", "per5"])
@pytest.mark.parametrize("n_in", [100, 513, 4200])
def test_plan_with_4_to_8_coordinates_equals_the_sort(n_in, form):
    """space_dim > 3 always takes select_rows_stream8 + neighbors_kernel8 (LDS transposition up to 4096 keys, the kernel's own
    count atomics beyond), with or without PIT_PLAN_TWO_PASSES."""
    for n, (kind, k, want_cap) in enumerate((("cloud", 9, "fit"), ("dups", 14, 16), ("grid", 2, "fit"), ("hits", 0, 1), ("same", 1, "fit"))):
        c = Case(kind, form, 2, 37, n_in, seed=70 + n_in + n)
        run_wave_case(c, k, want_cap, (c.id, "k", k, "cap", want_cap))


@gpu
@pytest.mark.parametrize("form", ["euc2", "per3", "euc8"])
@pytest.mark.parametrize("n_in", [65, 1025, 4097])
def test_neighbors_fwd_lists_the_set_of_the_statistics_it_is_given(n_in, form):
    """pit_neighbors_fwd called directly (neighbors_kernel, neighbors_kernel8) on the reference's statistics: the list depends on
    stats[1] alone - rows 0 and 2 are handed over as NaN."""
    for n, (kind, k, want_cap) in enumerate((("dups", 14, 16), ("cloud", 5, "fit"), ("grid", n_in - 1, "fit"))):
        c = Case(kind, form, 3, 21, n_in, seed=40 + n_in + n)
        want, member, count = c.ref(k)
        cap = cap_for(count, want_cap)
        assert_reference_conditions(count, cap, want_cap, c.id)
        stats = want.clone()
        stats[0] = stats[2] = float("nan")
        for rev in (False, True):
            o = dev_neighbors(c, stats, cap, rev)
            check_lists_ordered(o, member, count, cap, (c.id, k, cap, rev))
            if rev:
                check_transpose(o["idx"], o["cnt"], cap, o["rev_ptr"], o["rev_row"], c.n_in, (c.id, k, cap))


# =========================================================================== 3. pit_plan_fwd, a row per lane
def subset_rows(c, k, seed):
    """Rows of a sample compared with the CPU sort: the first and the last workgroup (256 rows), up to 300 rows built next to a
    tie shell of more than 40 keys (plan_rows_fix redoes them), 2000 rows drawn with a fixed seed."""
    g = torch.Generator().manual_seed(seed)
    redo = (c.near > 40).nonzero().reshape(-1)[:300]
    last0 = (c.n_out - 1) // 256 * 256
    rows = torch.cat([torch.arange(256), torch.arange(last0, c.n_out), redo, torch.randperm(c.n_out, generator=g)[:2000]])
    return torch.unique(rows), redo


def run_lane_case(c, k, cap, rev, expect_lane, overflow, seed=5, all_redone=False):
    """flags = 0 against PIT_PLAN_WAVE_PER_ROW on all rows (on the device), and against the CPU sort on subset_rows.
    all_redone: every row has more than 40 candidates, so plan_rows_fix rewrites every list in ascending order and the output
    cannot tell which kernel ran (all keys identical; any rank_k >= 39, whose lists hold k + 2 > 40 keys)."""
    what = (c.id, "k", k, "cap", cap, "rev", rev)
    assert lane_expected(c.b, c.n_out, c.n_in, c.coords, k, rev, 0) == expect_lane, what
    d = dev_plan(c, k, cap, rev, 0, to_cpu=False)
    w = dev_plan(c, k, cap, rev, WAVE_PER_ROW, to_cpu=False)
    # which kernel ran
    assert all_ascending(w["idx"], w["cnt"], cap), what
    assert all_ascending(d["idx"], d["cnt"], cap) == (not expect_lane or all_redone), what
    # every row: statistics and counts bit for bit, lists as sorted sets (rows within cap)
    assert torch.equal(bits(d["stats"]), bits(w["stats"])), what
    assert torch.equal(d["cnt"], w["cnt"]), what
    fits = (d["cnt"] <= cap).unsqueeze(-1)
    ds, ws = masked(d["idx"], d["cnt"], cap, BIG).sort(-1).values, masked(w["idx"], w["cnt"], cap, BIG).sort(-1).values
    assert bool(((ds == ws) | ~fits).all()), what
    rows, redo = subset_rows(c, k, seed)
    want, member, count = c.ref(k, rows)
    if redo.numel():                                             # rows the lane kernel cannot hold: more than 40 keys <= m_(k+1) <= U
        at = torch.searchsorted(rows, redo)
        le = (c.m(rows)[:, at] <= want[1][:, at].unsqueeze(-1)).sum(-1)
        assert bool((le > 40).any()), what
    if overflow:
        assert int(count.max()) > cap and int(count.min()) <= cap, (what, int(count.min()), int(count.max()))
    else:
        assert int(count.max()) <= cap, (what, int(count.max()))
    dc = {n: v.cpu() for n, v in d.items() if n != "ws"}
    check_stats(dc["stats"][:, :, rows], want, what)
    check_lists_as_sets(dc["idx"][:, rows], dc["cnt"][:, rows], member, count, cap, what)
    if rev:
        check_transpose(dc["idx"], dc["cnt"], cap, dc["rev_ptr"], dc["rev_row"], c.n_in, what)
        wc = {n: v.cpu() for n, v in w.items() if n != "ws"}
        check_transpose(wc["idx"], wc["cnt"], cap, wc["rev_ptr"], wc["rev_row"], c.n_in, what)
        if not overflow:                                         # (an overflowed row's first cap entries are other keys in block order)
            assert torch.equal(dc["rev_ptr"], wc["rev_ptr"]), what
    return dc


# (id, kind, form, n_out per sample, n_in, rank_k, cap, overflow?)   plan_rows_fix<4> <= 256 keys < <16> <= 1024 keys < <64>
LANE_CASES = [
    ("euc2-fix4", "dups", "euc2", 16384, 200, 5, 64, False),
    ("euc1-fix64", "dups", "euc1", 16500, 1100, 9, 64, True),
    ("euc3-fix16", "dups", "euc3", 16500, 600, 20, 128, False),
    ("per1-fix16", "dups", "per1", 16384, 600, 3, 64, True),
    ("per1of2-hits", "hits", "per1of2", 16384, 256, 7, 16, False),
    ("per2-fix64", "dups", "per2", 16500, 1100, 12, 128, False),
    ("per3-fix4", "dups", "per3", 16384, 200, 5, 16, True),
    ("euc2-cloud", "cloud", "euc2", 16500, 600, 17, 24, False),
    ("euc3-hits", "hits", "euc3", 16384, 200, 0, 8, False),
    ("euc2-grid", "grid", "euc2", 16500, 1000, 2, 8, False),      # (rank 2: a node's 5 / a centre's 4 nearest; larger shells overflow every lane)
    ("per2-same-fix4", "same", "per2", 16384, 130, 4, 130, False),
    ("euc2-tiny", "tiny", "euc2", 16384, 600, 4, 64, False),
]


@gpu
@pytest.mark.parametrize("rev", [False, True], ids=["norev", "rev"])
@pytest.mark.parametrize("case", LANE_CASES, ids=[c[0] for c in LANE_CASES])
def test_lane_per_row_plan_equals_the_sort_and_the_wave_per_row_plan(case, rev):
    """All four plan_rows_lane instances (Euclidean / periodic x at most two / three coordinates; periodic with three
    coordinates is PIT_METRIC_PERIODIC2D at space_dim 3, which the entry accepts) and all three plan_rows_fix instances, at
    2 x 16384 rows (the rows >= 32768 edge) and 2 x 16500 (a partial last workgroup); every n_in but 256 leaves padding keys."""
    _, kind, form, n_out, n_in, k, cap, overflow = case
    c = Case(kind, form, 2, n_out, n_in, seed=300 + n_in + k)
    run_lane_case(c, k, cap, rev, True, overflow, all_redone=kind == "same")


@gpu
@pytest.mark.parametrize("edge", ["rows-16383", "rank-62", "rank-63", "lds2d-3712", "lds2d-3713", "lds3d-2816", "lds3d-2817",
                                  "one-sample"])
def test_lane_per_row_plan_host_edges(edge):
    """Each side of every host condition of the lane kernel, the kernel that ran read off the list order."""
    if edge == "rows-16383":
        run_lane_case(Case("dups", "euc2", 2, 16383, 200, seed=1), 5, 32, True, False, True)
    elif edge == "one-sample":                                   # mesh_batch = 1 keeps the wave kernel at any row count
        run_lane_case(Case("cloud", "euc2", 1, 33000, 200, seed=2), 5, 8, False, False, False)
    elif edge.startswith("rank"):
        k = int(edge[5:])
        run_lane_case(Case("dups", "euc2", 2, 16384, 200, seed=3), k, 128, True, k == 62, False, all_redone=True)
    elif edge.startswith("lds2d"):
        n_in = int(edge[6:])
        run_lane_case(Case("cloud", "euc2", 2, 16500, n_in, seed=4), 10, 16, True, n_in == 3712, False, seed=6)
        if n_in == 3713:                                         # (without lists a 2-coordinate mesh never reaches the limit)
            run_lane_case(Case("cloud", "euc2", 2, 16384, n_in, seed=4), 10, 16, False, True, False, seed=6)
    else:
        n_in = int(edge[6:])
        run_lane_case(Case("cloud", "euc3", 2, 16500, n_in, seed=5), 10, 16, False, n_in == 2816, False, seed=6)


# =========================================================================== 4. transposed lists
# (mesh_batch, n_out, n_in, kind, rank_k, cap wanted): 127 / 128 / 129 / 257 rows around NBR_ROWS = 128, 255 / 256 / 257 / 513 keys
# around the scan's 256-key chunks, 4096 keys: the last size with LDS histograms
TRANSPOSE_CASES = [(1, 127, 255, "cloud", 6, "fit"), (3, 128, 256, "dups", 2, 4), (1, 129, 257, "grid", 9, "fit"),
                   (3, 257, 513, "dups", 14, 16), (3, 129, 4096, "dups", 5, "fit"), (1, 257, 256, "hits", 0, 1),
                   (3, 127, 513, "same", 3, "fit"), (1, 128, 4096, "dups", 14, 16)]


def transpose_id(t):
    return f"b{t[0]}-N{t[1]}-J{t[2]}-{t[3]}-cap{t[5]}"


@functools.lru_cache(maxsize=2)
def lists_case(t):
    """Lists of the wave-per-row plan built without reverse lists, checked against the sort."""
    b, n_out, n_in, kind, k, want_cap = t
    c = Case(kind, "euc2", b, n_out, n_in, seed=900 + n_out + n_in)
    want, member, count = c.ref(k)
    cap = cap_for(count, want_cap)
    assert_reference_conditions(count, cap, want_cap, c.id)
    o = dev_plan(c, k, cap, False, 0)
    check_stats(o["stats"], want, c.id)
    check_lists_ordered(o, member, count, cap, c.id)
    return c, k, cap, o


@gpu
@pytest.mark.parametrize("t", TRANSPOSE_CASES, ids=transpose_id)
def test_lists_transpose_equals_a_cpu_transposition(t):
    """pit_lists_transpose (nbr_count_lds, nbr_scan_kernel, nbr_fill_lds) called twice on the same dirty workspace and rev_row."""
    c, k, cap, o = lists_case(t)
    rc, d = dev_transpose(c, o["idx"], o["cnt"], cap)
    assert rc == 0
    first = {n: v.cpu() for n, v in d.items()}
    check_transpose(o["idx"], o["cnt"], cap, first["rev_ptr"], first["rev_row"], c.n_in, (c.id, "first call"))
    rc, d = dev_transpose(c, o["idx"], o["cnt"], cap, bufs=d)    # the buffers as the first call left them
    assert rc == 0
    check_transpose(o["idx"], o["cnt"], cap, d["rev_ptr"].cpu(), d["rev_row"].cpu(), c.n_in, (c.id, "second call"))
    assert torch.equal(d["rev_ptr"].cpu(), first["rev_ptr"])


@gpu
@pytest.mark.parametrize("t", [TRANSPOSE_CASES[3], (1, 9000, 3, "grid", 0, 2)], ids=transpose_id)
def test_lists_sort_ranges_orders_every_range_with_the_empty_slots_last(t):
    """pit_lists_sort_ranges on two overflow cases: every key's range ascending, its -1 slots last, the same entries.  The second
    (three keys listed by 9000 rows) has ranges of more than 4096 entries: the kernel's rank sort instead of its LDS sort."""
    from position_induced_transformer_amd import _lib
    c, k, cap, o = lists_case(t)
    rc, d = dev_transpose(c, o["idx"], o["cnt"], cap)
    assert rc == 0
    assert bool((d["rev_row"] == -1).any()) and int((o["cnt"] > cap).sum()) > 0
    srt = torch.full_like(d["rev_row"], -1)
    rc = _lib.lib().pit_lists_sort_ranges(d["rev_ptr"].data_ptr(), d["rev_row"].data_ptr(), c.b, c.n_in, c.n_out * cap,
                                          srt.data_ptr(), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    srt, p = srt.cpu(), d["rev_ptr"].cpu()
    assert (int((p[:, 1:] - p[:, :-1]).max()) > 4096) == (c.n_in == 3)
    check_transpose(o["idx"], o["cnt"], cap, p, srt, c.n_in, (c.id, "sorted"))
    for s in range(c.b):
        total = int(p[s, c.n_in])
        keyid = torch.repeat_interleave(torch.arange(c.n_in), (p[s, 1:] - p[s, :-1]).long())
        u = srt[s, :total].long() & 0xFFFFFFFF                   # as unsigned: -1 is the largest
        key = keyid * (1 << 33) + u
        assert bool((key[1:] >= key[:-1]).all()), (c.id, s)


@gpu
def test_lists_transpose_refuses_more_than_4096_keys():
    c = Case("cloud", "euc2", 1, 9, 4097, seed=1)
    idx, cnt = torch.zeros(1, 9, 4, dtype=torch.int32), torch.full((1, 9), 4, dtype=torch.int32)
    rc, _ = dev_transpose(c, idx, cnt, 4)
    assert rc == ERR_UNSUPPORTED


@gpu
@pytest.mark.parametrize("n_in", [4097, 5000])
@pytest.mark.parametrize("want_cap", ["fit", 16], ids=["fit", "cap16"])
def test_plan_with_reverse_lists_beyond_4096_keys(n_in, want_cap):
    """Counts from neighbors_kernel's own atomics, nbr_scan_kernel, nbr_fill_kernel; 3 samples x 129 rows, with overflowed rows
    (cap 16) and without; called twice on the same buffers."""
    c = Case("dups", "euc3", 3, 129, n_in, seed=n_in)
    want, member, count = c.ref(14)
    cap = cap_for(count, want_cap)
    assert_reference_conditions(count, cap, want_cap, c.id)
    bufs = plan_buffers(c, cap, True)
    for call in (1, 2):
        o = dev_plan(c, 14, cap, True, 0, bufs=bufs)
        check_stats(o["stats"], want, (c.id, call))
        check_lists_ordered(o, member, count, cap, (c.id, call))
        check_transpose(o["idx"], o["cnt"], cap, o["rev_ptr"], o["rev_row"], c.n_in, (c.id, call))


# =========================================================================== the reference itself (CPU)
def test_reference_distances_are_the_oracles_and_its_candidate_set_holds_every_kept_key():
    """`sqdist` above equals pit_oracle's three distance functions bit for bit (the period taken from the mesh as the oracle
    does), and the reference candidate set contains the oracle's kept set (attention_weights > 0) for head scales from 1e-3
    to 1e3, on a random cloud and on a grid with tie shells."""
    g = torch.Generator().manual_seed(3)
    side = 12
    j = torch.arange(side * side)
    grid = torch.stack([j % side, j // side], -1).float() / side
    cloud = torch.rand(150, 2, generator=g)
    for mesh_in in (cloud, grid):
        mesh_out = torch.cat([mesh_in[::5], torch.rand(31, 2, generator=g)])
        assert torch.equal(sqdist(EUC, mesh_out[None], mesh_in[None], 0.0)[0], orc.sqdist_euclid(mesh_out, mesh_in))
        l1, l2 = float(orc.period_1d(mesh_in)), float(orc.period_2d(mesh_in))
        assert torch.equal(sqdist(P1, mesh_out[None], mesh_in[None], l1)[0], orc.sqdist_periodic1d(mesh_out, mesh_in))
        assert torch.equal(sqdist(P2, mesh_out[None], mesh_in[None], l2)[0], orc.sqdist_periodic2d(mesh_out, mesh_in))
        for metric, period in ((EUC, 0.0), (P2, l2)):
            m = sqdist(metric, mesh_out[None], mesh_in[None], period)[0]
            for locality in (0.02, 0.2):
                k, _ = orc.quantile_rank(locality, m.shape[1])
                _, member, count = ref_rows(m, k)
                assert int(count.min()) >= min(k + 2, m.shape[1])
                c = torch.tensor([1e-3, 0.7, 1e3]).reshape(3, 1, 1)
                kept = orc.attention_weights(m, c, locality, batched=False) > 0
                assert kept.any(-1).all() and bool((member[None] | ~kept).all()), (metric, locality)
