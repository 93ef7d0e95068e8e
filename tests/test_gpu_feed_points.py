"""GPU: the subsampling feed - ops.batch_feed_points (pit_batch_feed_points) against its host restatement
(engine.feed_points / DeviceFeed.expected_points) bit for bit, and engine.DeviceFeed(subsample=True) inside captured steps.

The launch moves words, so every comparison of data is equality of int32 words: destination point k of slot s is source point
``feed_points(L, m, seed, epoch, idx, group)[k]`` of sample idx, points beyond min(m, L) are zero words, and the words around
every destination keep their sentinel.  Source words have the top two bits of each half clear (finite as fp32 and as two bf16) and the source padding holds a NaN
word, so a NaN in a destination can only have come from beyond a sample's length.  The model-level comparisons use the
project's 1e-5: a captured step against an eager forward and loss of a twin with the same weights on the same buffers."""
import pytest
import torch

from test_gpu_feed import expect

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
NAN_WORD = 0x7FC00001
FINITE = 0x3FFF3FFF                                                   # a word under this mask is finite as fp32 and as two bf16
KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "i32": torch.int32}      # bf16: two channels per word
TOL = 1e-5


def _guarded(count, pad=4):
    buf = torch.full((pad + count + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[pad:pad + count]


class Group:
    """One cloud of a synthetic dataset: ``N`` samples of ``n`` points, fields of ``words`` int32 per point viewed as their
    dtype, optional lengths (points beyond hold the NaN word), and for each field a destination of (batch, m) points with
    sentinel words around it."""

    def __init__(self, g, N, batch, n, m, fields, lens, gen, len_dst=True, table=True):
        self.g, self.n, self.m, self.batch = g, n, m, batch
        self.lens = lens                                              # as given (the launch clamps into [1, n])
        self.L = [min(max(int(v), 1), n) for v in lens] if lens is not None else [n] * N
        self.lens_dev = torch.tensor([int(v) for v in lens], dtype=torch.int32).cuda() if lens is not None else None
        self.host, self.src, self.bufs, self.dst = [], [], [], []
        for j, (words, kind) in enumerate(fields):
            w = torch.randint(0, 2 ** 30, (N, n, words), generator=gen, dtype=torch.int64).to(torch.int32) & FINITE
            for i, length in enumerate(self.L):
                w[i, length:] = NAN_WORD
            off = (j + g) % 4                                         # (sources and destinations at every residue mod 16 bytes)
            store = torch.zeros(off + w.numel(), dtype=torch.int32)
            store[off:] = w.reshape(-1)
            self.host.append(w)
            self.src.append(store.cuda()[off:].view(N, n, words).view(KINDS[kind]))
            buf, view = _guarded(batch * m * words, pad=4 + (3 * j + g) % 5)
            self.bufs.append(buf)
            self.dst.append(view.view(batch, m, words).view(KINDS[kind]))
        self.len_buf, self.len_dst = _guarded(batch) if len_dst else (None, None)
        self.table_buf, table = _guarded(batch * m) if table else (None, None)
        self.table = table.view(batch, m) if table is not None else None

    def check(self, idx, seed, epoch, what):
        from position_induced_transformer_amd.engine import feed_points
        pts = [feed_points(self.L[i], self.m, seed, epoch, i, self.g) for i in idx]
        for w, buf, dst in zip(self.host, self.bufs, self.dst):
            rows = torch.zeros((self.batch, self.m, w.shape[-1]), dtype=torch.int32)
            for s, (i, p) in enumerate(zip(idx, pts)):
                rows[s, :p.numel()] = w[i][p]
            want = torch.full((buf.numel(),), SENTINEL, dtype=torch.int32)
            pad = (buf.numel() - rows.numel()) // 2
            want[pad:pad + rows.numel()] = rows.reshape(-1)
            got = buf.cpu()
            assert torch.equal(got, want), what + (w.shape[-1],)     # the points, the zeros beyond, the sentinels around
            assert not bool((got == NAN_WORD).any()), what
            if dst.is_floating_point():
                assert not bool(torch.isnan(dst.float()).any()), what
        if self.len_buf is not None:
            want = torch.full((self.len_buf.numel(),), SENTINEL, dtype=torch.int32)
            want[4:4 + self.batch] = torch.tensor([p.numel() for p in pts], dtype=torch.int32)
            assert torch.equal(self.len_buf.cpu(), want), what
        if self.table_buf is not None:
            rows = torch.full((self.batch, self.m), -1, dtype=torch.int32)
            for s, p in enumerate(pts):
                rows[s, :p.numel()] = p.to(torch.int32)
            want = torch.full((self.table_buf.numel(),), SENTINEL, dtype=torch.int32)
            want[4:4 + rows.numel()] = rows.reshape(-1)
            assert torch.equal(self.table_buf.cpu(), want), what
        return pts


class Case:
    def __init__(self, N, batch, groups, seed=0x1234567_89ABCDEF, gen_seed=5, whole_words=0):
        """groups: per group dict(n, m, fields=[(words, kind)], lens=None | 'random' | list, len_dst, table)."""
        self.N, self.batch, self.seed = N, batch, seed
        gen = torch.Generator().manual_seed(gen_seed)
        self.groups = []
        for g, spec in enumerate(groups):
            lens = spec.get("lens")
            if lens == "random":
                lens = torch.randint(1, spec["n"] + 1, (N,), generator=gen).tolist()
                lens[0] = spec["n"]                                   # a full cloud among them
            self.groups.append(Group(g, N, batch, spec["n"], spec["m"], spec["fields"], lens, gen,
                                     spec.get("len_dst", True), spec.get("table", True)))
        self.whole = None
        if whole_words:                                               # a whole-row field beside the point fields
            self.whole_src = torch.randint(0, 2 ** 30, (N, whole_words), generator=gen, dtype=torch.int64).to(torch.int32).cuda()
            self.whole_buf, view = _guarded(batch * whole_words)
            self.whole = view.view(batch, whole_words)
        from position_induced_transformer_amd import ops
        self.state = ops.new_feed_state("cuda")
        self.indices = torch.full((batch,), -5, dtype=torch.int32, device="cuda")
        self.n_valid = torch.full((1,), -5, dtype=torch.int32, device="cuda")

    def launch(self, world=1, rank=0, drop_last=True, shuffle=True, order=None):
        from position_induced_transformer_amd import ops
        src = [t for grp in self.groups for t in grp.src] + ([self.whole_src] if self.whole is not None else [])
        dst = [t for grp in self.groups for t in grp.dst] + ([self.whole] if self.whole is not None else [])
        kinds = [1 + grp.g for grp in self.groups for _ in grp.src] + ([0] if self.whole is not None else [])
        both = self.groups + [None] * (2 - len(self.groups))
        ops.batch_feed_points(src, dst, kinds, self.state, rank, world, drop_last, shuffle, order, self.seed, self.indices,
                              self.n_valid, [grp.lens_dev if grp else None for grp in both],
                              [grp.len_dst if grp else None for grp in both], [grp.table if grp else None for grp in both])

    def check(self, cursor, world=1, rank=0, drop_last=True, shuffle=True, order=None):
        idx, nv, steps = expect(self.N, self.batch, world, rank, int(drop_last), shuffle, order, self.seed, cursor)
        what = (self.N, self.batch, cursor, world, rank, drop_last, shuffle)
        assert self.indices.tolist() == idx and int(self.n_valid) == nv, what
        assert self.state.tolist() == [cursor + 1, 0], what
        if self.whole is not None:
            want = torch.full((self.whole_buf.numel(),), SENTINEL, dtype=torch.int32)
            want[4:4 + self.whole.numel()] = self.whole_src.cpu()[torch.tensor(idx)].reshape(-1)
            assert torch.equal(self.whole_buf.cpu(), want), what
        return [grp.check(idx, self.seed, cursor // steps, what + (grp.g,)) for grp in self.groups]

    def bits(self):
        return [b.clone() for grp in self.groups for b in grp.bufs + [grp.len_buf, grp.table_buf] if b is not None]


FIELDS0 = [(1, "i32"), (2, "bf16"), (3, "f32"), (11, "f32"), (44, "f32")]     # words per point 1, 2, 3, 11, 44
FIELDS1 = [(3, "bf16"), (1, "f32")]


# --------------------------------------------------------------------------- the launch against the host restatement
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 17, 64, 65, 257, 1000])
def test_subsets_match_the_host_bit_for_bit(n):
    """n points, m in {1, n - 1, n}, batches 1, 3 and 8, five fields of group 0 and two of group 1 in one launch; lengths in
    [1, n] (so m passes some samples' lengths), out-of-range lengths clamped, and a group without lengths."""
    for m in sorted({1, max(n - 1, 1), n}):
        for batch in (1, 3, 8):
            lens1 = None if batch == 3 else "random"
            case = Case(11, batch, [dict(n=n, m=m, fields=FIELDS0, lens="random"), dict(n=n, m=m, fields=FIELDS1, lens=lens1)],
                        gen_seed=n * 31 + m)
            if batch == 8:                                            # clamped where they are read
                case.groups[0].lens_dev[1:3] = torch.tensor([0, n + 3], dtype=torch.int32)
                case.groups[0].L[1:3] = [1, n]
                fill = torch.Generator().manual_seed(n)
                for w, src in zip(case.groups[0].host, case.groups[0].src):   # (sample 2 now counts n points: no padding)
                    w[2] = torch.randint(0, 2 ** 30, w[2].shape, generator=fill, dtype=torch.int64).to(torch.int32) & FINITE
                    src.view(torch.int32)[2] = w[2].cuda()
            steps = 11 // batch
            for cursor in (0, steps + 1):                             # two epochs
                case.state[0] = cursor
                case.launch()
                pts0, pts1 = case.check(cursor)
                if n >= 5 and m == n and lens1 is None:               # (full clouds of >= 5 points: the two groups differ)
                    assert any(a.tolist() != b.tolist() for a, b in zip(pts0, pts1))


def test_a_point_that_straddles_two_pieces():
    """m = 4099 points of 3 words: the pieces of 2048 words cut through points; with and without lengths."""
    for lens in (None, "random"):
        case = Case(5, 3, [dict(n=4100, m=4099, fields=[(3, "f32")], lens=lens)])
        for cursor in (0, 1):
            case.launch()
            case.check(cursor)


def test_above_the_small_launch_tier():
    """batch 8, m = 8192 of n = 16384 points, 9 words (and a 1-word field whose piece holds four chunks of indices): the
    1024-thread form, lengths from 4096."""
    lens = [4096 + 1365 * i for i in range(9)]                        # 4096 .. 15016: three clouds shorter than m
    case = Case(9, 8, [dict(n=16384, m=8192, fields=[(9, "f32"), (1, "i32")], lens=lens)])
    case.launch()
    pts, = case.check(0)
    assert min(p.numel() for p in pts) < 8192 and max(p.numel() for p in pts) == 8192


@pytest.mark.parametrize("mode", ["identity", "order", "order_out_of_range", "two_ranks", "partly_filled"])
def test_sample_choice_is_the_plain_feeds(mode):
    """shuffle=False, a caller's order (entries out of range are clamped), two ranks, drop_last=False: the slots hold the
    samples pit_batch_feed would choose; a whole-row field travels beside the point fields."""
    N, batch = 11, 4
    order = None
    if mode.startswith("order"):
        order = torch.randperm(N, generator=torch.Generator().manual_seed(9))
        if mode == "order_out_of_range":
            order[::3] = torch.tensor([-1, N, -2 ** 31, 2 ** 31 - 1])
    order_dev = order.to(torch.int32).cuda() if order is not None else None
    world = 2 if mode == "two_ranks" else 1
    drop_last = mode != "partly_filled"
    for rank in range(world):
        case = Case(N, batch, [dict(n=65, m=16, fields=[(2, "f32"), (3, "i32")], lens="random"),
                               dict(n=17, m=17, fields=[(1, "f32")], lens="random")], whole_words=5)
        steps = N // (batch * world) if drop_last else -(-N // (batch * world))
        for cursor in range(steps + 1):
            case.launch(world, rank, drop_last, mode != "identity", order_dev)
            case.check(cursor, world, rank, drop_last, mode != "identity", order)


def test_two_launches_at_one_cursor_give_the_same_bits():
    case = Case(11, 3, [dict(n=257, m=64, fields=FIELDS0, lens="random"), dict(n=65, m=64, fields=FIELDS1, lens="random")])
    case.state[0] = 7
    case.launch()
    first = case.bits()
    case.check(7)
    case.state[0] = 2
    case.launch()
    assert any(not torch.equal(a, b) for a, b in zip(first, case.bits()))
    case.state[0] = 7
    case.launch()
    assert all(torch.equal(a, b) for a, b in zip(first, case.bits()))


# --------------------------------------------------------------------------- engine.DeviceFeed(subsample=True)
LENGTHS = [96, 40, 77, 58, 91, 64, 45, 83, 70, 52, 96, 61]           # 12 clouds of width 96, lengths in [40, 96]
WIDTH = 96


def _model(seed=0):
    from position_induced_transformer_amd import tasks
    torch.manual_seed(seed)
    return tasks.pit_cloud_fps(2, 3, 1, 32, 2, 1, 16, 0.25, 0.25).cuda()


@pytest.fixture(scope="module")
def clouds():
    """mesh (12, 96, 2), func (12, 96, 3), target (12, 96, 1), lengths; NaN beyond every length."""
    from position_induced_transformer_amd import tasks
    mesh, func, target, lens = tasks.ragged_clouds(LENGTHS, WIDTH, channels=3, seed=41, device="cuda", pad_value=float("nan"))
    return {"mesh_in": mesh, "func_in": func, "target": target, "len_in": lens}


def _batch(m, batch=4, two_clouds=False):
    mesh = torch.zeros(batch, m, 2, device="cuda")
    return mesh, torch.zeros(batch, m, 3, device="cuda"), (torch.zeros(batch, m, 2, device="cuda") if two_clouds else mesh), \
        torch.zeros(batch, m, 1, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gathered(feed, data, cursor):
    """The host-gathered batch of the launch at ``cursor``: per field the (batch, m, c) tensor of src[idx][points], zero
    beyond, and per group the lengths min(m, L)."""
    idx, nv = feed.expected_indices(cursor)
    pts = feed.expected_points(cursor)
    one_cloud = pts[1] is None
    out = {}
    for name in ("mesh_in", "func_in", "mesh_out", "target"):
        if name not in data:
            continue
        p = pts[0 if one_cloud or name in ("mesh_in", "func_in") else 1]
        m = feed.m_in if one_cloud or name in ("mesh_in", "func_in") else feed.m_out
        rows = torch.zeros((feed.batch, m) + tuple(data[name].shape[2:]), dtype=data[name].dtype, device="cuda")
        for s, (i, q) in enumerate(zip(idx, p)):
            rows[s, :q.numel()] = data[name][i][q.cuda()]
        out[name] = rows
    out["lens"] = [[q.numel() for q in p] if p is not None else None for p in pts]
    out["idx"], out["n_valid"] = idx, nv
    return out


def _check_feed(feed, step, data, cursor):
    want = _gathered(feed, data, cursor)
    assert feed.indices.tolist() == want["idx"] and int(feed.cursor) == cursor + 1, cursor
    for name in ("mesh_in", "func_in", "mesh_out", "target"):
        if name in data:
            assert torch.equal(_bits(getattr(step, name)), _bits(want[name])), (cursor, name)
            assert not bool(torch.isnan(getattr(step, name)).any()), (cursor, name)
    for table, p, m in ((feed.points_in, feed.expected_points(cursor)[0], feed.m_in),
                        (feed.points_out, feed.expected_points(cursor)[1], feed.m_out)):
        if p is not None:
            assert table.tolist() == [q.tolist() + [-1] * (m - q.numel()) for q in p], cursor
    return want


def test_one_cloud_gives_target_the_subset_of_mesh_in(clouds):
    """mesh_out IS mesh_in: one group; the static lengths receive min(m, L) and the rows beyond are zero."""
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    step = EvalStep(_model(), _batch(64), 1, 2, len_in=[64] * 4)
    feed = DeviceFeed(step, clouds, seed=9, subsample=True, drop_last=False)
    assert feed.points_out is None and feed.kinds == [1, 1, 1]
    for cursor in range(4):                                           # an epoch of three launches and the next one's first
        feed.launch()
        want = _check_feed(feed, step, clouds, cursor)
        assert step.len_in.tolist() == want["lens"][0] == [min(64, LENGTHS[i]) for i in want["idx"]]
        assert int(step.n_valid) == 4
        for s, length in enumerate(want["lens"][0]):
            assert not bool(_bits(step.mesh_in[s, length:]).any()) and not bool(_bits(step.target[s, length:]).any())
    assert any(length < 64 for length in LENGTHS)                     # (the case has clouds shorter than the step)


def test_two_clouds_get_different_subsets(clouds):
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    data = {**clouds, "mesh_out": clouds["mesh_in"].clone(), "len_out": clouds["len_in"].clone()}
    step = EvalStep(_model(), _batch(32, two_clouds=True), 1, 2)
    feed = DeviceFeed(step, data, seed=9, subsample=True)             # a step without lengths: 32 <= the shortest cloud (40)
    assert feed.kinds == [1, 2, 1, 2] and feed.points_in.shape == feed.points_out.shape == (4, 32)
    for cursor in range(3):
        feed.launch()
        _check_feed(feed, step, data, cursor)
        assert all(a != b for a, b in zip(feed.points_in.tolist(), feed.points_out.tolist()))
        assert int(feed.points_in.min()) >= 0 and int(feed.points_out.min()) >= 0


def test_a_graph_replayed_across_three_epochs(clouds):
    """The launch alone in a graph: every replay draws the subsets of its position, epoch after epoch."""
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    step = EvalStep(_model(), _batch(64), 1, 2, len_in=[64] * 4)
    feed = DeviceFeed(step, clouds, seed=21, subsample=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        feed.launch()
        feed.seek(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        feed.launch()
    assert int(feed.cursor) == 0
    tables = []
    for cursor in range(3 * feed.steps_per_epoch):
        graph.replay()
        want = _check_feed(feed, step, clouds, cursor)
        assert step.len_in.tolist() == want["lens"][0]
        tables.append(dict(zip(want["idx"], feed.points_in.tolist())))
    epochs = [{k: v for t in tables[e * 3:e * 3 + 3] for k, v in t.items()} for e in range(3)]
    assert all(sorted(e) == list(range(12)) for e in epochs)          # every cloud once per epoch
    assert all(epochs[0][i] != epochs[1][i] != epochs[2][i] for i in range(12))      # with a new subset in each


def test_seek_and_resume_continue_with_the_same_subsets(clouds):
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    a_step = EvalStep(_model(), _batch(64), 1, 2, len_in=[64] * 4)
    a = DeviceFeed(a_step, clouds, seed=33, subsample=True)
    for cursor in (7, 0, 4):
        a.seek(cursor)
        a.launch()
        _check_feed(a, a_step, clouds, cursor)
    state = a.state_dict()
    assert state["cursor"] == 5 and state["subsample"] is True and state["m_in"] == 64 and state["n_in"] == 96
    b_step = EvalStep(_model(), _batch(64), 1, 2, len_in=[64] * 4)
    b = DeviceFeed(b_step, clouds, seed=33, subsample=True)
    b.load_state_dict(state)
    for cursor in (5, 6):
        a.launch()
        b.launch()
        _check_feed(b, b_step, clouds, cursor)
        for name in ("mesh_in", "func_in", "target", "len_in"):
            assert torch.equal(_bits(getattr(a_step, name)), _bits(getattr(b_step, name))), (cursor, name)
        assert torch.equal(a.points_in, b.points_in)
    other = DeviceFeed(EvalStep(_model(), _batch(32), 1, 2), clouds, seed=33, subsample=True)
    with pytest.raises(ValueError, match="m_in"):
        other.load_state_dict(state)


# --------------------------------------------------------------------------- model level
def _twin_loss(twin, weights, step, lengths=None):
    """The eager forward and loss of ``twin`` with the given weights on the step's static buffers."""
    from position_induced_transformer_amd import ops, utils
    twin.load_state_dict(weights)
    ops.parameters_changed()
    with torch.no_grad():
        if lengths is None:
            return float(utils.RelLpNorm(1, 2)(step.target, twin(step.mesh_in, step.func_in, step.mesh_in)))
        pred = twin(step.mesh_in, step.func_in, step.mesh_in, len_in=lengths)
        return float(utils.RelLpNorm(1, 2)(step.target, pred, lengths))


def _captured_train_step(clouds, m, with_lengths):
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    model = _model()
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = FlatAdam(flat, lr=1e-3, cosine_t_max=100)
    step = TrainStep(model, _batch(m), 1, 2, optimizer=opt, flat=flat, **({"len_in": [m] * 4} if with_lengths else {}))
    feed = DeviceFeed(step, clouds, seed=17, subsample=True)
    step.capture(warmup=1)
    return step, feed, _model()


def test_train_step_without_lengths_on_subsets(clouds):
    """m = 32 <= the shortest cloud: a rectangular step, FlatAdam in the graph.  After every replay of two epochs the static
    buffers equal the host-gathered batch, and the step's loss an eager forward and loss on those buffers with the weights
    the replay started from."""
    step, feed, twin = _captured_train_step(clouds, 32, False)
    assert step.len_in is None and int(feed.cursor) == 0 and feed.steps_per_epoch == 3
    for cursor in range(6):
        weights = {k: v.detach().clone() for k, v in step.model.state_dict().items()}
        step.replay()
        want = _check_feed(feed, step, clouds, cursor)
        assert want["lens"][0] == [32] * 4
        ref = _twin_loss(twin, weights, step)
        got = float(step.loss)
        print(f"cursor {cursor}: loss {got:.7f} eager {ref:.7f}")
        assert got == got and abs(got - ref) <= TOL * abs(ref), (cursor, got, ref)
    assert int(feed.cursor) == 6


def test_train_step_with_lengths_on_subsets(clouds):
    """m = 64 with len_in: the static lengths are min(L, 64), the rows beyond are zero, and the loss is finite and equals the
    eager ragged forward on the host-gathered batch and lengths."""
    step, feed, twin = _captured_train_step(clouds, 64, True)
    for cursor in range(6):
        weights = {k: v.detach().clone() for k, v in step.model.state_dict().items()}
        step.replay()
        want = _check_feed(feed, step, clouds, cursor)
        lengths = [min(LENGTHS[i], 64) for i in want["idx"]]
        assert step.len_in.tolist() == lengths == want["lens"][0]
        for s, length in enumerate(lengths):
            for t in (step.mesh_in, step.func_in, step.target):
                assert not bool(_bits(t[s, length:]).any()), (cursor, s)
        ref = _twin_loss(twin, weights, step, lengths)
        got = float(step.loss)
        print(f"cursor {cursor}: loss {got:.7f} eager {ref:.7f}")
        assert torch.isfinite(step.loss).all() and abs(got - ref) <= TOL * abs(ref), (cursor, got, ref)


@pytest.mark.parametrize("count", [12, 10])
def test_eval_step_on_subsets_counts_the_valid_samples(clouds, count):
    """drop_last=False: the launch writes n_valid, the metric counts the valid samples (12: three full batches; the first 10
    clouds: the last batch holds two)."""
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    data = {k: v[:count] for k, v in clouds.items()}
    step = EvalStep(_model(), _batch(32), 1, 2, capacity=count)
    feed = DeviceFeed(step, data, shuffle=False, drop_last=False, seed=3, subsample=True)
    assert feed.steps_per_epoch == 3
    step.reset()
    for cursor in range(3):
        step.run_eager()
        want = _check_feed(feed, step, data, cursor)
        assert int(step.n_valid) == want["n_valid"] == min(4, count - 4 * cursor)
    res = step.result()
    assert res.count == count and res.rel_lp == res.rel_lp and res.rel_lp > 0
