"""GPU: ragged batches on the candidate-list layers (pit_distlist_*_ragged_*, ops.ListPlan(len_out=, len_in=),
metric.forward_list / forward with lengths, pit_metric(len_in=), engine.TrainStep(len_in=)).

The contract: sample s of the padded batch comes out as the EXISTING list layer computes that cloud alone - lists
idx[s, :len_out[s]], values [s, :len_in[s]], n_in = len_in[s].  Outputs, d(values) and d(sqd) are compared with that run as bits
(N <= 512 rows: no key exceeds a chunk of d(values)); d(lmda), which meets in fp64 slots, with the fp64 sum of the per-sample
values at LMDA_TOL.  An independent fp64 oracle on the dense matrix of each trimmed sample (test_gpu_distlist._oracle_layer)
bounds both.  Tolerances are the project's (test_gpu_shared_latent): none is new."""
import pytest
import torch

from test_gpu_distlist import _check, _hub_lists, _oracle_layer
from test_gpu_mesh_grad import _err
from test_gpu_shared_latent import FWD_TOL, GRAD_TOL, LMDA_TOL

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _sample_lists(lo, li, cap, q, g, garbage):
    """Lists of one cloud of ``lo`` rows over ``li`` keys: per row between min(list_capacity, li, cap) and min(cap, li) valid
    slots at random positions, distinct keys, distances with injected ties; the other slots are padding - with ``garbage`` keys
    -1, li (a key that is real for a wider sample of the batch) and 2^31 - 1 with NaN distances, otherwise -1 and 0."""
    from position_induced_transformer_amd import metric
    need, top = min(metric.list_capacity(q, li), li, cap), min(cap, li)
    idx = torch.empty(lo, cap, dtype=torch.int64)
    sqd = torch.rand(lo, cap, generator=g)
    for r in range(lo):
        nv = int(torch.randint(need, top + 1, (1,), generator=g))
        slots = torch.randperm(cap, generator=g)
        idx[r, slots[:nv]] = torch.randperm(li, generator=g)[:nv]
        if nv > 4:
            sqd[r, slots[1:1 + nv // 4]] = float(sqd[r, slots[0]])
            sqd[r, slots[nv - 1]] = float(sqd[r, slots[nv // 2]])
        pad = slots[nv:]
        idx[r, pad] = torch.tensor([-1, li, 2 ** 31 - 1])[(r + torch.arange(len(pad))) % 3] if garbage else -1
        sqd[r, pad] = NAN if garbage else 0.0
    return idx, sqd


class Batch:
    """A padded ragged batch for one layer: the trimmed samples and their padded stack.  ``noisy``: NaN in padded value rows,
    padded d_out rows and the padding slots' sqd, and random keys with NaN distances as the lists of padded rows; otherwise
    zeros and -1."""

    def __init__(self, form, heads, dim, cap, q, n, j, len_out, len_in, seed, noisy=True, hub=False):
        self.concat = form == "self"
        self.heads, self.dim, self.cap, self.q, self.n, self.j = heads, dim, cap, q, n, j
        self.len_out, self.len_in = list(len_out), list(len_in)
        b = self.b = len(len_out)
        g = torch.Generator().manual_seed(seed)
        width = (heads + (1 if self.concat else 0)) * dim
        fill = NAN if noisy else 0.0
        # (the keys of padded rows come from a generator of their own: the real part is the same with and without noise)
        self.idx = torch.randint(0, j, (b, n, cap), generator=torch.Generator().manual_seed(seed + 1000)) if noisy \
            else torch.full((b, n, cap), -1, dtype=torch.int64)
        self.sqd = torch.full((b, n, cap), fill)
        self.x = torch.full((b, j, dim), fill)
        self.dy = torch.full((b, n, width), fill)
        self.alone = []
        for s in range(b):
            lo, li = self.len_out[s], self.len_in[s]
            i_s, s_s = _hub_lists(lo, cap, seed + s) if hub else _sample_lists(lo, li, cap, q, g, noisy)
            x_s, dy_s = torch.randn(1, li, dim, generator=g), torch.randn(1, lo, width, generator=g)
            self.idx[s, :lo], self.sqd[s, :lo], self.x[s, :li], self.dy[s, :lo] = i_s, s_s, x_s[0], dy_s[0]
            self.alone.append((i_s, s_s, x_s, dy_s))

    def layer(self, seed=0):
        from position_induced_transformer_amd import metric
        torch.manual_seed(seed)
        return (metric.posatt_metric if self.concat else metric.posatt_cross_metric)(self.heads, self.dim, self.q).cuda()

    def run_ragged(self, mod, lengths=True):
        from position_induced_transformer_amd import ops
        s1, x1 = self.sqd.cuda().requires_grad_(True), self.x.cuda().requires_grad_(True)
        mod.lmda.grad = None
        kw = {}
        if lengths:
            kw = dict(lengths=self.len_in) if self.concat else dict(len_out=self.len_out, len_in=self.len_in)
        with ops.head_scale_route("host"):
            out = mod.forward_list(self.idx.cuda(), s1, x1, **kw)
            out.backward(self.dy.cuda())
        return out.detach(), x1.grad, mod.lmda.grad.clone(), s1.grad

    def run_alone(self, mod, s):
        """The existing layer on the trimmed tensors of sample s (lists shared by its batch of one)."""
        from position_induced_transformer_amd import ops
        i_s, s_s, x_s, dy_s = self.alone[s]
        s1, x1 = s_s.cuda().requires_grad_(True), x_s.cuda().requires_grad_(True)
        mod.lmda.grad = None
        with ops.head_scale_route("host"):
            out = mod.forward_list(i_s.cuda(), s1, x1)
            out.backward(dy_s.cuda())
        return out.detach()[0], x1.grad[0], mod.lmda.grad.clone(), s1.grad

    def check_padding_is_zero(self, got, tag):
        out, dv, _, dsq = got
        d = self.dim
        for s in range(self.b):
            lo, li = self.len_out[s], self.len_in[s]
            heads_cols = out[s, lo:, (d if self.concat else 0):]
            assert not bool(heads_cols.any()) and bool(torch.isfinite(heads_cols).all()), (tag, s, "out")
            if self.concat:                                              # the copied input columns as they are, NaN included
                assert torch.equal(_bits(out[s, lo:, :d]), _bits(self.x[s, lo:].cuda())), (tag, s, "copied inputs")
            assert bool((_bits(dv[s, li:]) == 0).all()), (tag, s, "d_values of padding keys")
            assert bool((_bits(dsq[s, lo:]) == 0).all()), (tag, s, "d_sqd of padded rows")
            pad = ~((self.idx[s, :lo] >= 0) & (self.idx[s, :lo] < li))
            assert not bool(dsq[s, :lo].cpu()[pad].any()), (tag, s, "d_sqd of padding slots")


def _lmda_err(got, ref):
    """max |err| / max |ref|; a reference that is an exact 0 (one kept slot per row: sqd - mbar = 0 in every term) asks for an
    exact 0."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    if float(ref.abs().max()) == 0.0:
        return float(got.abs().max())
    return float((got - ref).abs().max() / ref.abs().max())


# (form, heads, dim, cap, q, N, J, len_out, len_in); the self form has N == J and one length per sample
CASES = [
    ("cross", 1, 8, 1, 1.0, 150, 400, (150, 77, 1), (400, 333, 1)),
    ("self", 2, 6, 1, 1.0, 300, 300, (300, 131, 1), (300, 131, 1)),
    ("cross", 2, 16, 64, 0.05, 150, 400, (150, 77, 1), (400, 50, 301)),
    ("self", 3, 5, 64, 0.05, 300, 300, (300, 131, 2), (300, 131, 2)),
    ("cross", 3, 7, 65, 0.05, 150, 400, (9, 150, 80), (129, 400, 64)),
    ("self", 1, 12, 65, 0.1, 300, 300, (300, 65, 1), (300, 65, 1)),
    ("cross", 2, 4, 300, 0.3, 512, 400, (512, 77, 300), (400, 333, 1)),
    ("self", 2, 9, 300, 0.3, 300, 300, (299, 300, 40), (299, 300, 40)),
]
IDS = [f"{c[0]}-h{c[1]}-d{c[2]}-k{c[3]}-q{c[4]}" for c in CASES]
_RUNS = {}


def _case_runs(i):
    """One ragged run and the cloud-alone runs of a case, shared by the tests that read them."""
    if i not in _RUNS:
        c = CASES[i]
        batch = Batch(*c, seed=300 + i)
        mod = batch.layer(i)
        _RUNS[i] = (batch, mod, batch.run_ragged(mod), [batch.run_alone(mod, s) for s in range(batch.b)])
    return _RUNS[i]


# --------------------------------------------------------------------------- 1. the cloud alone
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_sample_is_the_cloud_alone(i):
    batch, mod, got, alone = _case_runs(i)
    out, dv, dl, dsq = got
    assert out.shape == (batch.b, batch.n, (batch.heads + (1 if batch.concat else 0)) * batch.dim)
    assert dv.shape == batch.x.shape and dsq.shape == batch.sqd.shape
    for s, (o_s, dv_s, _, dsq_s) in enumerate(alone):
        lo, li = batch.len_out[s], batch.len_in[s]
        assert torch.equal(_bits(out[s, :lo]), _bits(o_s)), (IDS[i], s, "out")
        assert torch.equal(_bits(dv[s, :li]), _bits(dv_s)), (IDS[i], s, "d_values")
        assert torch.equal(_bits(dsq[s, :lo]), _bits(dsq_s)), (IDS[i], s, "d_sqd")
    ref = sum(a[2].double() for a in alone)
    e = _lmda_err(dl, ref)
    print(IDS[i], "d_lmda vs the fp64 sum of the per-sample values:", e)
    assert e <= LMDA_TOL
    batch.check_padding_is_zero(got, IDS[i])


# --------------------------------------------------------------------------- 2. the fp64 oracle
@pytest.mark.parametrize("i", [2, 3, 4, 7], ids=[IDS[i] for i in (2, 3, 4, 7)])
def test_every_sample_matches_the_fp64_oracle(i):
    """An independent dense fp64 restatement per trimmed sample; the real parts of the batch are joined into one tensor each
    (max |err| / max |ref| per tensor), d(lmda) is the sum over the samples."""
    batch, mod, got, _ = _case_runs(i)
    refs = [_oracle_layer(i_s, s_s, batch.len_in[s], x_s, dy_s, mod.lmda, batch.q, batch.concat) for s, (i_s, s_s, x_s, dy_s) in enumerate(batch.alone)]
    flat = lambda parts: torch.cat([p.reshape(-1).double().cpu() for p in parts])
    lens = list(zip(batch.len_out, batch.len_in))
    got_real = (flat(got[0][s, :lo] for s, (lo, _) in enumerate(lens)), flat(got[1][s, :li] for s, (_, li) in enumerate(lens)), got[2],
                flat(got[3][s, :lo] for s, (lo, _) in enumerate(lens)))
    ref_real = (flat(r[0] for r in refs), flat(r[1] for r in refs), sum(r[2] for r in refs), flat(r[3] for r in refs), sum(r[4] for r in refs))
    _check(got_real, ref_real, IDS[i])


# --------------------------------------------------------------------------- 3. padding is inert
@pytest.mark.parametrize("i", [2, 3], ids=[IDS[2], IDS[3]])
def test_padding_is_inert(i):
    """NaN in padded value rows, padded d_out rows, the padding slots' sqd and the lists of padded rows (random keys, NaN
    distances) against zeros and -1: the real part keeps its bits, padded rows and keys come out exactly zero."""
    noisy, clean = Batch(*CASES[i], seed=300 + i, noisy=True), Batch(*CASES[i], seed=300 + i, noisy=False)
    assert bool(torch.isnan(noisy.x).any()) and bool(torch.isnan(noisy.dy).any()) and bool(torch.isnan(noisy.sqd).any())
    mod = noisy.layer(i)
    a, b = noisy.run_ragged(mod), clean.run_ragged(mod)
    for s in range(noisy.b):
        lo, li = noisy.len_out[s], noisy.len_in[s]
        ok = (noisy.idx[s, :lo] >= 0) & (noisy.idx[s, :lo] < li)
        assert torch.equal(ok, (clean.idx[s, :lo] >= 0) & (clean.idx[s, :lo] < li))          # the same real slots in both
        assert torch.equal(_bits(a[0][s, :lo]), _bits(b[0][s, :lo])) and torch.equal(_bits(a[1][s, :li]), _bits(b[1][s, :li]))
        assert torch.equal(_bits(a[3][s, :lo]), _bits(b[3][s, :lo]))
    assert bool(torch.isfinite(a[2]).all()) and _lmda_err(a[2], b[2]) <= LMDA_TOL
    noisy.check_padding_is_zero(a, "noisy")
    clean.check_padding_is_zero(b, "clean")


# --------------------------------------------------------------------------- 4. full lengths
@pytest.mark.parametrize("form", ["cross", "self"])
def test_full_lengths_give_the_dense_entries_bits(form):
    n, j = (150, 400) if form == "cross" else (300, 300)
    batch = Batch(form, 2, 16, 64, 0.05, n, j, (n,) * 3, (j,) * 3, seed=41)
    mod = batch.layer(1)
    a, b = batch.run_ragged(mod), batch.run_ragged(mod, lengths=False)
    for t in (0, 1, 3):
        assert torch.equal(_bits(a[t]), _bits(b[t])), t
    assert _lmda_err(a[2], b[2]) <= LMDA_TOL


# --------------------------------------------------------------------------- 5. a hub key
def test_a_hub_key_agrees_with_the_cloud_alone():
    """600 rows that all list key 0: its range takes more than one chunk of d(values), summed by separate waves."""
    batch = Batch("cross", 2, 16, 8, 1.0, 600, 40, (600, 550), (40, 33), seed=51, hub=True)
    mod = batch.layer(2)
    got = batch.run_ragged(mod)
    for s in range(batch.b):
        o_s, dv_s, _, dsq_s = batch.run_alone(mod, s)
        lo, li = batch.len_out[s], batch.len_in[s]
        assert torch.equal(_bits(got[0][s, :lo]), _bits(o_s)) and torch.equal(_bits(got[3][s, :lo]), _bits(dsq_s))
        e = _err(got[1][s, :li], dv_s)
        print("hub key, sample", s, "d_values vs the cloud alone:", e)
        assert e <= GRAD_TOL
    batch.check_padding_is_zero(got, "hub")


# --------------------------------------------------------------------------- 6. reproducibility
def test_two_runs_give_the_same_bits():
    batch = Batch(*CASES[4], seed=61)
    mod = batch.layer(3)
    a = batch.run_ragged(mod)
    (torch.randn(512, 512, device="cuda") @ torch.randn(512, 512, device="cuda")).sum().item()       # unrelated device work in between
    b = batch.run_ragged(mod)
    for t in (0, 1, 3):
        assert torch.equal(_bits(a[t]), _bits(b[t])), t
    assert _err(a[2], b[2]) <= 1e-6                                      # (d(scale) meets in fp64 slots: order-free up to the last bits)


# --------------------------------------------------------------------------- 7. capture
def test_a_captured_layer_follows_lengths_overwritten_in_place():
    """Selection, forward and backward in one graph; the lengths are overwritten between replays and the transposed index - built
    once from the keys against the padded width - stays the plan's."""
    from position_induced_transformer_amd import ops
    form, heads, dim, cap, q, n, j, len_out, len_in = CASES[2]
    batch = Batch(form, heads, dim, cap, q, n, j, (n,) * 3, (j,) * 3, seed=71, noisy=False)        # every slot of every row is real
    idx, dy = batch.idx.cuda(), batch.dy.cuda()
    sets = [(len_out, len_in), ((40, 150, 99), (400, 70, 222)), ((n,) * 3, (j,) * 3)]
    lo_t = torch.tensor(sets[0][0], dtype=torch.int32, device="cuda")
    li_t = torch.tensor(sets[0][1], dtype=torch.int32, device="cuda")
    s1, x1 = batch.sqd.cuda().requires_grad_(True), batch.x.cuda().requires_grad_(True)
    c = torch.tensor([11.0, 6.0], device="cuda").requires_grad_(True)
    plan = ops.ListPlan(idx, s1, j, q, len_out=lo_t, len_in=li_t)

    def step(ss, xx, cc, pl):
        ss.grad = xx.grad = cc.grad = None
        pl.refresh()                                                     # the selection reads the lengths: part of the step
        out = ops.posatt_list_apply(xx, cc, pl, heads, head_is_scale=True, sqd=ss)
        out.backward(dy)
        return out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s1, x1, c, plan)                                            # warm-up outside the capture (workspaces, the transposed index)
    torch.cuda.current_stream().wait_stream(side)
    rev = plan.transposed()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(s1, x1, c, plan)
    for t in (1, 2, 0):
        lo_t.copy_(torch.tensor(sets[t][0], dtype=torch.int32)); li_t.copy_(torch.tensor(sets[t][1], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert plan.transposed() is rev
        s_e, x_e, c_e = s1.detach().clone().requires_grad_(True), x1.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
        out_e = step(s_e, x_e, c_e, ops.ListPlan(idx, s_e, j, q, len_out=list(sets[t][0]), len_in=list(sets[t][1])))
        assert torch.equal(_bits(out), _bits(out_e)) and torch.equal(_bits(x1.grad), _bits(x_e.grad)) and torch.equal(_bits(s1.grad), _bits(s_e.grad)), t
        assert _err(c.grad, c_e.grad) <= 1e-6                            # (d(scale) meets in fp64 slots)


# --------------------------------------------------------------------------- 8. the model
WIDTH, LATENT = 200, 48
FIRST, SECOND = [200, 131, 64], [64, 200, 177]


def _model(seed=0):
    from position_induced_transformer_amd import metric
    torch.manual_seed(seed)
    ltt = torch.rand(LATENT, 2)
    return metric.pit_metric(2, 1, 1, 32, 2, 2, ltt, 0.1, 0.1, sqdist=metric.sqdist_periodic_box((1.0, None)), learn_latent=True,
                             neighbors="auto", builder="hip").cuda()


def _clouds(lengths, seed):
    """Random clouds in the unit square (no ties: the lists of the padded batch and of a trimmed cloud keep the same pairs),
    NaN in every padded point, input and target value."""
    g = torch.Generator().manual_seed(seed)
    b = len(lengths)
    mesh, func, target = torch.rand(b, WIDTH, 2, generator=g), torch.randn(b, WIDTH, 1, generator=g), torch.randn(b, WIDTH, 1, generator=g)
    for s, n in enumerate(lengths):
        mesh[s, n:] = NAN; func[s, n:] = NAN; target[s, n:] = NAN
    return mesh.cuda(), func.cuda(), target.cuda()


def _grads(model):
    return {k: q.grad.detach().clone() for k, q in model.named_parameters()}


def _per_sample(model, mesh, func, weight, lengths):
    """The model on every trimmed cloud alone: predictions, the summed gradients of sum(pred * weight), the summed cut_rows."""
    preds, cuts = [], [0, 0]
    model.zero_grad(set_to_none=True)
    for s, n in enumerate(lengths):
        m = mesh[s:s + 1, :n].contiguous()
        p = model(m, func[s:s + 1, :n].contiguous(), m)
        (p * weight[s:s + 1, :n]).sum().backward()
        preds.append(p.detach()[0])
        cuts[0] += int(model.down.last_lists.cut_rows); cuts[1] += int(model.up.last_lists.cut_rows)
    return preds, _grads(model), cuts


def _check_grads(got, ref, tag):
    for k in ref:
        e = _err(got[k], ref[k])
        print(tag, "grad", k, e)
        assert e <= (LMDA_TOL if k.endswith("lmda") else GRAD_TOL), (tag, k)


def test_model_on_a_ragged_batch_is_the_sum_of_its_clouds():
    model = _model()
    mesh, func, _ = _clouds(FIRST, 81)
    weight = torch.randn(3, WIDTH, 1, generator=torch.Generator().manual_seed(82)).cuda()
    preds, ref, cuts = _per_sample(model, mesh, func, weight, FIRST)
    model.zero_grad(set_to_none=True)
    out = model(mesh, func, mesh, len_in=FIRST)
    assert out.shape == (3, WIDTH, 1) and bool(torch.isfinite(out).all())
    assert [int(model.down.last_lists.cut_rows), int(model.up.last_lists.cut_rows)] == cuts
    loss = sum((out[s, :n] * weight[s, :n]).sum() for s, n in enumerate(FIRST))
    loss.backward()
    for s, n in enumerate(FIRST):
        e = _err(out[s, :n], preds[s])
        print("sample", s, "prediction vs the cloud alone:", e)
        assert e <= FWD_TOL
    got = _grads(model)
    assert "mesh_ltt" in got and bool(torch.isfinite(got["mesh_ltt"]).all()) and bool(got["mesh_ltt"].any())
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    _check_grads(got, ref, "eager")


def test_captured_train_step_serves_two_length_sets():
    from position_induced_transformer_amd import engine
    model = _model(1)
    mesh, func, target = _clouds(FIRST, 91)
    step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, len_in=FIRST)
    assert step._len_loss is step.len_in
    step.capture(warmup=1)
    twin = _model(1)
    for lengths, seed in ((SECOND, 92), (FIRST, 91)):
        m, f, t = _clouds(lengths, seed)
        step.set_batch(f, t, mesh_in=m, len_in=lengths)
        step.replay()
        torch.cuda.synchronize()
        eager = engine.TrainStep(twin, (m, f, m, t), 1, 2, len_in=lengths)
        eager.run_eager()
        torch.cuda.synchronize()
        for s, n in enumerate(lengths):
            assert _err(step.out[s, :n], eager.out[s, :n]) <= FWD_TOL, (lengths, s)
        assert bool(torch.isfinite(step.loss)) and abs(float(step.loss) - float(eager.loss)) <= FWD_TOL * abs(float(eager.loss))
        _check_grads(_grads(model), _grads(twin), f"captured {lengths}")
