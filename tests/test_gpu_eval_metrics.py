"""pit_eval_metrics (csrc/pit_eval.hip) through ops.eval_metrics, against an fp64 evaluation of utils.py:59-98 on the CPU from the
same fp32 inputs: the shape grid, every dispatch instance, lengths and n_valid over NaN-filled padding, the cursor over several
launches, capacity overflow between guard rows, the arrival ticket, and bit-for-bit repeatability.

Dispatch instances: a (sample, channel) series is split over EVAL_PARTS = 1, 2, 4, ..., 64 workgroups; the count doubles while
each part keeps >= 1024 points and fewer than 512 workgroups exist (``parts_rule`` below re-computes the rule, and every case
asserts that the library - through its workspace size - agrees).  Instance k >= 2 is first reached at npts = 1024 * k.

Inputs are built as in tests/test_gpu_reductions.py: |true| in [0.25, 1.25), |true - pred'| in [0.05, 0.55).
Bounds: the project's for these reductions against fp64 - sums and table entries 2e-6 relative, the RelMax quantities 1e-6;
the stored prediction is bit-equal to torch-CPU ``pred*scale + shift``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_LOSS, TOL_MAX = 2e-6, 1e-6
NAN = float("nan")
SENTINEL = -7.25
EVAL_PARTS = (1, 2, 4, 8, 16, 32, 64)


def parts_rule(batch, npts, nch):
    parts = 1
    while parts < 64 and batch * nch * parts < 512 and npts // (2 * parts) >= 1024:
        parts *= 2
    return parts


@functools.lru_cache(maxsize=8)
def case(batch, npts, nch, affine, seed=0):
    """fp32 inputs, computed once per case and never modified."""
    g = torch.Generator().manual_seed(17 + 1000 * seed + npts % 997 + 7 * batch + 3 * nch + (500 if affine else 0))
    u = lambda *s: torch.rand(*s, generator=g)                        # noqa: E731
    sgn = lambda: torch.where(u(batch, npts, nch) < 0.5, -1.0, 1.0)   # noqa: E731
    t = sgn() * (0.25 + u(batch, npts, nch))
    qq = t + sgn() * (0.05 + 0.5 * u(batch, npts, nch))
    sc = sh = None
    q = qq
    if affine:
        sc, sh = 0.5 + u(npts, nch), 2.0 * u(npts, nch) - 1.0
        q = (qq - sh) / sc
    return t, q, sc, sh


def reference(t, q, sc, sh, p, lens=None, n_valid=None):
    """(RelLp_s, RelMax_s) per valid sample in fp64, and pred' as torch-CPU fp32 forms it."""
    b, npts, nch = t.shape
    q32 = q * sc + sh if sc is not None else q
    q64 = q.double() * sc.double() + sh.double() if sc is not None else q.double()
    t64 = t.double()
    lp, mx = [], []
    for s in range(b if n_valid is None else n_valid):
        n = npts if lens is None else lens[s]
        d, tt = (t64[s, :n] - q64[s, :n]), t64[s, :n]
        lp.append(float((torch.norm(d, p=p, dim=0) / torch.norm(tt, p=p, dim=0)).mean()))
        mx.append(float((d.abs().max(dim=0).values / tt.abs().max(dim=0).values).mean()))
    return torch.tensor(lp, dtype=torch.float64), torch.tensor(mx, dtype=torch.float64), q32


class Outputs:
    """State, table and store of a pass, the two optional outputs between guard rows that keep a sentinel."""

    def __init__(self, capacity, npts, nch, cols=None):
        from position_induced_transformer_amd import ops
        self.state = ops.new_eval_state("cuda")
        mid = () if cols is None else (cols,)
        self.table_all = torch.full((capacity + 2,) + mid + (2,), SENTINEL, device="cuda")
        self.store_all = torch.full((capacity + 2,) + mid + (npts, nch), SENTINEL, device="cuda")
        self.table, self.store = self.table_all[1:-1], self.store_all[1:-1]

    def guards_intact(self):
        return all(bool((x[0] == SENTINEL).all()) and bool((x[-1] == SENTINEL).all()) for x in (self.table_all, self.store_all))


def launch(out, t, q, sc, sh, p, lens=None, n_valid=None, advance=True, table=None, store=None, store_true=False, fill=None):
    """One launch; ``fill``: what padded points and skipped samples hold on the device.  Asserts that the ticket is left zero."""
    from position_induced_transformer_amd import ops
    b, npts, nch = t.shape
    t, q = t.clone(), q.clone()
    if fill is not None:
        for s in range(b):
            n = 0 if (n_valid is not None and s >= n_valid) else (npts if lens is None else lens[s])
            t[s, n:] = fill
            q[s, n:] = fill
    dev = lambda x: None if x is None else x.cuda()                   # noqa: E731
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device="cuda")
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    ops.eval_metrics(t.cuda(), q.cuda(), nch, p, out.state, dev(sc), dev(sh), lengths=ln, n_valid=nv,
                     per_sample=out.table if table is None else table, pred_store=out.store if store is None else store,
                     advance=advance, store_true=store_true)
    assert ops.eval_parts(b, npts, nch) == parts_rule(b, npts, nch)
    ws = ops._EVAL_WS[ops._ws_key(torch.device("cuda", torch.cuda.current_device()))]
    assert int(ws.view(torch.int32)[0]) == 0, "the arrival ticket must be left zero"


def close(got, want, tol):
    got, want = torch.as_tensor(got, dtype=torch.float64).cpu(), torch.as_tensor(want, dtype=torch.float64)
    return bool(((got - want).abs() <= tol * want.abs()).all())


def check_single_launch(b, npts, nch, p, affine):
    t, q, sc, sh = case(b, npts, nch, affine)
    lp, mx, q32 = reference(t, q, sc, sh, p)
    out = Outputs(b, npts, nch)
    launch(out, t, q, sc, sh, p)
    st = out.state.cpu()
    assert close(st[0], lp.sum(), TOL_LOSS), (float(st[0]), float(lp.sum()))
    assert close(st[1], mx.sum(), TOL_MAX), (float(st[1]), float(mx.sum()))
    assert close(st[2], lp.max(), TOL_LOSS) and close(st[3], mx.max(), TOL_MAX)
    assert st[4] == b and st[5] == 1 and st[6] == 0 and st[7] == 0
    assert close(out.table[:, 0], lp, TOL_LOSS) and close(out.table[:, 1], mx, TOL_MAX)
    assert torch.equal(out.store.cpu(), q32)
    assert out.guards_intact()


# --------------------------------------------------------------------------- the shape grid
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("npts", [1, 63, 64, 65, 257, 4099])
def test_grid_against_fp64(npts, nch, b, p, affine):
    check_single_launch(b, npts, nch, p, affine)


# --------------------------------------------------------------------------- every dispatch instance, at its first size and one past
INSTANCE_SHAPES = [(1, 2047, 1, 1)] + [(1, 1024 * k + extra, 1, k) for k in EVAL_PARTS[1:] for extra in (0, 1)] + \
                  [(2, 2048, 3, 2), (2, 2049, 3, 2), (5, 4096, 3, 4), (171, 2048, 3, 1), (170, 2048, 3, 2)]


@pytest.mark.parametrize("b,npts,nch,parts", INSTANCE_SHAPES, ids=[f"b{b}-n{n}-c{c}-parts{k}" for b, n, c, k in INSTANCE_SHAPES])
def test_every_dispatch_instance(b, npts, nch, parts):
    assert parts_rule(b, npts, nch) == parts
    if parts > 1:
        assert parts_rule(b, 1024 * parts - 1, nch) == parts // 2     # one point fewer takes the instance below
    check_single_launch(b, npts, nch, 2, affine=(npts % 2 == 1))


def test_instances_cover_the_list():
    assert {k for _, _, _, k in INSTANCE_SHAPES} == set(EVAL_PARTS)
    assert parts_rule(10, 177241, 1) == 64                             # the ZSSR shape: 640 workgroups


# --------------------------------------------------------------------------- lengths and n_valid over NaN-filled padding
def lengths_for(b, npts):
    return ([npts, 1, 33 % npts + 1, max(1, npts // 2), max(1, npts - 1)] * b)[:b]


@pytest.mark.parametrize("n_valid", [0, 1, 5])
@pytest.mark.parametrize("npts,nch", [(1, 1), (65, 3), (257, 3), (4099, 1)])
def test_lengths_and_n_valid_never_read_padding(npts, nch, n_valid):
    b, p = 5, 2
    t, q, _, _ = case(b, npts, nch, False)
    lens = lengths_for(b, npts)
    lp, mx, _ = reference(t, q, None, None, p, lens, n_valid)
    got = {}
    for fill in (NAN, 0.0):
        out = Outputs(b, npts, nch)
        launch(out, t, q, None, None, p, lens=lens, n_valid=n_valid, fill=fill)
        got[fill == 0.0] = out
    a, z = got[False], got[True]
    for x, y in ((a.state, z.state), (a.table_all, z.table_all), (a.store_all, z.store_all)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    st = a.state.cpu()
    assert st[4] == n_valid and st[5] == 1
    if n_valid == 0:
        assert st[0] == 0 and st[1] == 0 and st[2] == 0 and st[3] == 0
    else:
        assert close(st[0], lp.sum(), TOL_LOSS) and close(st[1], mx.sum(), TOL_MAX)
        assert close(a.table[:n_valid, 0], lp, TOL_LOSS) and close(a.table[:n_valid, 1], mx, TOL_MAX)
    store = a.store.cpu()
    for s in range(b):
        if s < n_valid:
            assert torch.equal(store[s, :lens[s]], q[s, :lens[s]]) and bool((store[s, lens[s]:] == 0).all())
        else:                                                         # a skipped sample: no row written
            assert bool((store[s] == SENTINEL).all()) and bool((a.table[s] == SENTINEL).all())
    assert a.guards_intact()


# --------------------------------------------------------------------------- the cursor: three launches, overflow, advance = 0
def three_launches(b, npts, nch, p, capacity, valid=(None, 2, None)):
    out = Outputs(capacity, npts, nch)
    lp_all, mx_all, rows = [], [], []
    for i, nv in enumerate(valid):
        t, q, sc, sh = case(b, npts, nch, True, seed=i)
        lp, mx, q32 = reference(t, q, sc, sh, p, None, nv)
        launch(out, t, q, sc, sh, p, n_valid=nv, fill=NAN if nv is not None else None)
        lp_all.append(lp); mx_all.append(mx); rows.append(q32[:b if nv is None else nv])
    return out, torch.cat(lp_all), torch.cat(mx_all), torch.cat(rows)


@pytest.mark.parametrize("b,npts,nch", [(5, 65, 3), (5, 4099, 1)])
def test_three_launches_accumulate_and_are_repeatable(b, npts, nch):
    p, cap = 2, 16
    out, lp, mx, rows = three_launches(b, npts, nch, p, cap)
    n = 2 * b + 2
    st = out.state.cpu()
    assert st[4] == n and st[5] == 3
    assert close(st[0], lp.sum(), TOL_LOSS) and close(st[1], mx.sum(), TOL_MAX)
    assert close(st[2], lp.max(), TOL_LOSS) and close(st[3], mx.max(), TOL_MAX)
    assert close(out.table[:n, 0], lp, TOL_LOSS) and close(out.table[:n, 1], mx, TOL_MAX)       # rows at the running cursor
    assert torch.equal(out.store[:n].cpu(), rows)
    assert bool((out.table[n:] == SENTINEL).all()) and bool((out.store[n:] == SENTINEL).all())
    again, _, _, _ = three_launches(b, npts, nch, p, cap)             # a fresh (zeroed) state: the same bits
    assert torch.equal(again.state, out.state)
    assert torch.equal(again.table_all, out.table_all) and torch.equal(again.store_all, out.store_all)


def test_rows_past_the_capacity_are_not_written_but_counted():
    b, npts, nch, p, cap = 5, 65, 3, 2, 7
    out, lp, mx, rows = three_launches(b, npts, nch, p, cap)
    st = out.state.cpu()
    assert st[4] == 12 and close(st[0], lp.sum(), TOL_LOSS) and close(st[1], mx.sum(), TOL_MAX)
    assert close(out.table[:, 0], lp[:cap], TOL_LOSS) and torch.equal(out.store.cpu(), rows[:cap])
    assert out.guards_intact()


def test_advance_zero_leaves_the_cursor_and_columns_take_strided_rows():
    """The rollout's use: ``steps`` launches per batch into column t of a (capacity, steps, 2) table and a
    (capacity, steps, npts, nch) store, the last one moving the cursor."""
    b, npts, nch, p, steps, cap = 3, 65, 2, 2, 3, 8
    out = Outputs(cap, npts, nch, cols=steps)
    want_lp = torch.zeros(2 * b, steps, dtype=torch.float64)
    want_mx = torch.zeros(2 * b, steps, dtype=torch.float64)
    want_rows = torch.zeros(2 * b, steps, npts, nch)
    for rep in range(2):
        for k in range(steps):
            t, q, _, _ = case(b, npts, nch, False, seed=10 * rep + k)
            launch(out, q, t, None, None, p, advance=(k == steps - 1), table=out.table[:, k], store=out.store[:, k], store_true=True)
            assert out.state.cpu()[4] == (rep * b if k < steps - 1 else (rep + 1) * b)
            lp, mx, _ = reference(q, t, None, None, p)                # (the model output in the `true` slot)
            want_lp[rep * b:(rep + 1) * b, k], want_mx[rep * b:(rep + 1) * b, k] = lp, mx
            want_rows[rep * b:(rep + 1) * b, k] = q                   # store_true: the `true` slot is what is kept
    st = out.state.cpu()
    assert st[5] == 2 * steps and close(st[0], want_lp.sum(), TOL_LOSS) and close(st[1], want_mx.sum(), TOL_MAX)
    assert close(out.table[:2 * b, :, 0], want_lp, TOL_LOSS) and close(out.table[:2 * b, :, 1], want_mx, TOL_MAX)
    assert torch.equal(out.store[:2 * b].cpu(), want_rows)
    assert bool((out.table[2 * b:] == SENTINEL).all()) and out.guards_intact()


def test_wrapper_checks_on_device_tensors():
    from position_induced_transformer_amd import ops
    t = torch.zeros(2, 5, 1, device="cuda")
    state = ops.new_eval_state("cuda")
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.eval_metrics(t, t.clone().requires_grad_(True), 1, 2, state)
    with pytest.raises(RuntimeError, match="state must be"):
        ops.eval_metrics(t, t, 1, 2, torch.zeros(8, device="cuda"))
    with pytest.raises(RuntimeError, match="per_sample"):
        ops.eval_metrics(t, t, 1, 2, state, per_sample=torch.zeros(4, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="pred_store"):
        ops.eval_metrics(t, t, 1, 2, state, pred_store=torch.zeros(4, 6, 1, device="cuda"))
    with pytest.raises(RuntimeError, match="n_valid"):
        ops.eval_metrics(t, t, 1, 2, state, n_valid=torch.tensor([1], device="cuda"))
    assert float(state.abs().sum()) == 0.0                            # nothing was launched
