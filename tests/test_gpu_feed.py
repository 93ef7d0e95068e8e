"""GPU: the device-resident data feed - ops.batch_feed (pit_batch_feed) against its host restatement bit for bit, and
engine.DeviceFeed inside the captured steps against twins driven by set_batch.

The gather moves words, so every comparison of data is equality of int32 words.  The captured-step comparisons are equality of
bits too, and that is derived, not measured: under ops.reproducible() with every lmda frozen each sum on the path has a fixed
order, the kernels are deterministic, and a step fed by the feed sees exactly the inputs its twin receives through set_batch - a
difference means the feed delivered something else.  (The twins are brought to one state AFTER both captures: the warm-up passes
of a capture are real optimiser steps, on whatever each step's buffers held.)  The evaluation sums are fp64 sums over identical
per-sample terms; 1e-12 relative covers the association of the partial batches only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
NAN_WORDS = (0x7FC00001, 0x7F800001, -1, -0x00400000)               # quiet / signalling NaN payloads, as int32 words


# --------------------------------------------------------------------------- the host restatement of one launch
def expect(n, batch, world, rank, drop_last, shuffle, order, seed, cursor):
    """(indices, n_valid) of the launch at ``cursor`` (include/pit_hip.h), from engine.feed_order."""
    from position_induced_transformer_amd.engine import feed_order
    per = batch * world
    steps = n // per if drop_last else -(-n // per)
    epoch, i = divmod(cursor, steps)
    first = (i * world + rank) * batch
    pos = [(first + s) % n for s in range(batch)]
    if order is not None:
        idx = [min(max(int(order[g]), 0), n - 1) for g in pos]
    elif not shuffle:
        idx = pos
    else:
        perm = feed_order(n, seed, epoch).tolist()
        idx = [perm[g] for g in pos]
    return idx, min(max(n - first, 0), batch), steps


class Field:
    """A dataset field of ``n`` rows of ``words`` int32 at an offset of ``src_off`` words into its allocation, and its
    destination of ``batch`` rows ``pad`` words into a buffer of sentinel words."""

    def __init__(self, n, batch, words, src_off, pad, gen):
        raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (src_off + n * words,), dtype=torch.int64, generator=gen).to(torch.int32)
        k = raw.numel()
        for j, w in enumerate(NAN_WORDS):
            raw[j % k::7] = w if j % 2 else raw[j % k::7] | 0x7FC00000  # NaN bit patterns among the words
        self.store = raw.cuda()
        self.src = self.store[src_off:].view(n, words)
        self.pad, self.words, self.batch = pad, words, batch
        self.buf = torch.full((pad + batch * words + pad,), SENTINEL, dtype=torch.int32, device="cuda")
        self.dst = self.buf[pad:pad + batch * words].view(batch, words)
        self.want = self.buf.clone()

    def check(self, idx, what):
        self.want[self.pad:self.pad + self.batch * self.words] = self.src[torch.tensor(idx, device="cuda")].reshape(-1)
        assert torch.equal(self.buf, self.want), what                 # the rows, and the sentinel words around them


ROW_BYTES = (4, 12, 16, 7396, 65540)


@pytest.fixture(scope="module")
def fields37():
    gen = torch.Generator().manual_seed(5)
    # (source offsets and pads in words: every residue of source and destination mod 16 bytes occurs, congruent or not)
    return [Field(37, 8, rb // 4, off, pad, gen) for rb, off, pad in zip(ROW_BYTES, (0, 1, 4, 2, 3), (4, 5, 8, 7, 6))]


def _orders(n):
    g = torch.Generator().manual_seed(9)
    perm = torch.randperm(n, generator=g)
    wild = perm.clone()
    wild[::5] = torch.tensor([-1, n, -2 ** 31, 2 ** 31 - 1, n + 100, -7, 5, n - 1])[:len(wild[::5])]
    return perm, wild


MODES = ("identity", "feistel", "order", "order_out_of_range")


@pytest.mark.parametrize("drop_last", [1, 0])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_gather_matches_the_host_bit_for_bit(fields37, world, drop_last):
    from position_induced_transformer_amd import ops
    n, batch, seed = 37, 8, 0x1234567_89ABCDEF
    perm, wild = _orders(n)
    for mode in MODES:
        order = {"order": perm, "order_out_of_range": wild}.get(mode)
        order_dev = order.to(torch.int32).cuda() if order is not None else None
        for rank in range(world):
            state = ops.new_feed_state("cuda")
            indices = torch.full((batch,), -5, dtype=torch.int32, device="cuda")
            n_valid = torch.full((1,), -5, dtype=torch.int32, device="cuda")
            steps = expect(n, batch, world, rank, drop_last, mode != "identity", order, seed, 0)[2]
            for k in range(2 * steps + 1):
                ops.batch_feed([f.src for f in fields37], [f.dst for f in fields37], state, rank, world, bool(drop_last),
                               mode != "identity", order_dev, seed, indices, n_valid)
                idx, nv, _ = expect(n, batch, world, rank, drop_last, mode != "identity", order, seed, k)
                what = (mode, world, rank, drop_last, k)
                assert indices.tolist() == idx, what
                assert int(n_valid) == nv, what
                assert state.tolist() == [k + 1, 0], what
                for f in fields37:
                    f.check(idx, what + (f.words,))


def _simple_run(n, batch, world, words_list, launches, drop_last=1, shuffle=True, seed=3):
    from position_induced_transformer_amd import ops
    src = [(torch.arange(n * w, dtype=torch.int64) * 2654435761 % 2 ** 31).to(torch.int32).view(n, w).cuda() for w in words_list]
    for rank in range(world):
        bufs = [torch.full((batch * w + 8,), SENTINEL, dtype=torch.int32, device="cuda") for w in words_list]
        dst = [b[4:4 + batch * w].view(batch, w) for b, w in zip(bufs, words_list)]
        state, indices = ops.new_feed_state("cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")
        n_valid = torch.zeros(1, dtype=torch.int32, device="cuda")
        for k in range(launches):
            ops.batch_feed(src, dst, state, rank, world, bool(drop_last), shuffle, None, seed, indices, n_valid)
            idx, nv, _ = expect(n, batch, world, rank, drop_last, shuffle, None, seed, k)
            assert indices.tolist() == idx and int(n_valid) == nv and state.tolist() == [k + 1, 0], (rank, k)
            pick = torch.tensor(idx, device="cuda")
            for s_, d_, b_ in zip(src, dst, bufs):
                assert torch.equal(d_, s_[pick]), (rank, k)
                assert bool((b_[:4] == SENTINEL).all()) and bool((b_[-4:] == SENTINEL).all())


def _field_run(n, batch, row_bytes, offs, pads, launches, seed=13):
    """Fields at chosen source offsets and destination pads (words), compared whole - rows and sentinels - after every launch."""
    from position_induced_transformer_amd import ops
    gen = torch.Generator().manual_seed(seed)
    fields = [Field(n, batch, rb // 4, off, pad, gen) for rb, off, pad in zip(row_bytes, offs, pads)]
    state, indices = ops.new_feed_state("cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")
    for k in range(launches):
        ops.batch_feed([f.src for f in fields], [f.dst for f in fields], state, 0, 1, True, True, None, seed, indices, None)
        idx, _, _ = expect(n, batch, 1, 0, 1, True, None, seed, k)
        assert indices.tolist() == idx and state.tolist() == [k + 1, 0], k
        for f in fields:
            f.check(idx, (k, f.words))


# The entry has two forms (csrc/pit_feed.hip): 256-thread workgroups up to 2 MiB (524288 words) per launch, 1024-thread
# workgroups with pieces of at least 8192 words beyond.  Rows of 163844 and 327684 bytes (40961 and 81921 words: Vorticity's
# rows plus one word, so consecutive rows are 4 mod 16 apart and a slot's source and destination are congruent for one
# sample in four - both the 16-byte path with head and tail and the dword path occur in every launch, the source offsets and
# pads shift them against each other) move 614410 words at batch 5 and 7.9 M at batch 64:
#   batch 5   pieces of 8192 words, the last piece of either row ONE word; a piece is less than one tile
#   batch 64  pieces of 30724 words (two and three per row): several tiles per piece in both paths (8192 words as dwords, 16384 as 16-byte units)
@pytest.mark.parametrize("batch,launches", [(5, 3), (64, 2)])
def test_large_form_matches_the_host_bit_for_bit(batch, launches):
    assert (163844 + 327684) // 4 * batch > 524288                    # beyond the small form's limit
    _field_run(max(6, batch + 1), batch, (163844, 327684), (1, 2), (5, 7), launches)


@pytest.mark.parametrize("case", ["one_sample", "exactly_one_step", "batch_of_one", "cycle_walk_22_bits", "eight_fields"])
def test_edges(case):
    if case == "one_sample":
        _simple_run(1, 1, 1, [3], 3)
        _simple_run(1, 1, 1, [3], 3, drop_last=0)
    elif case == "exactly_one_step":
        _simple_run(24, 8, 3, [5, 1], 3)
        _simple_run(24, 8, 3, [5, 1], 3, drop_last=0)
    elif case == "batch_of_one":
        _simple_run(7, 1, 3, [2], 6)
        _simple_run(7, 1, 3, [2], 7, drop_last=0)
    elif case == "cycle_walk_22_bits":
        _simple_run((1 << 20) + 3, 8, 2, [1], 3)                      # 2^20 + 3 samples: a 22-bit domain, ~3/4 of it walked over
    else:
        _simple_run(11, 4, 1, [1, 2, 3, 4, 5, 6, 7, 8], 5, drop_last=0)


# --------------------------------------------------------------------------- engine.DeviceFeed in the captured steps
def _freeze(model):
    for name, q in model.named_parameters():
        if name.endswith("lmda"):
            q.requires_grad_(False)
    return model


def _fixed_model():
    from position_induced_transformer_amd import pit as P
    from position_induced_transformer_amd import tasks
    torch.manual_seed(3)
    model = tasks.pit_darcy(2, 1, 1, 16, 2, 2, tasks.grid_mesh_2d(4).cuda(), 0.2, 0.2).cuda()     # (pit_fixed with the Darcy forward)
    assert isinstance(model, P.pit_fixed)
    return _freeze(model)


def _fixed_data(n, seed=21):
    from position_induced_transformer_amd import tasks
    g = torch.Generator().manual_seed(seed)
    mesh = tasks.grid_mesh_2d(6).cuda()
    return mesh, torch.randn(n, 6, 6, 1, generator=g).cuda(), torch.randn(n, 6, 6, 1, generator=g).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _train_pair(with_adam, batch=4, n=20):
    """(step with a feed, its feed, twin step, x, y): two models from one seed, captured; then brought to ONE state."""
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    mesh, x, y = _fixed_data(n)
    steps = []
    for fed in (True, False):
        model = _fixed_model()
        flat = FlatGradients(model.parameters(), flatten_params=True)
        opt = FlatAdam(flat, lr=1e-3, cosine_t_max=10) if with_adam else None
        step = TrainStep(model, (mesh, x[:batch].clone(), mesh, y[:batch].clone()), 1, 2, optimizer=opt, flat=flat)
        feed = DeviceFeed(step, {"func_in": x, "target": y}, seed=17) if fed else None
        step.capture()
        steps.append((step, feed, flat, opt))
    (a, feed, flat_a, opt_a), (b, _, flat_b, opt_b) = steps
    flat_b.flat_params.copy_(flat_a.flat_params)
    flat_b.flat.copy_(flat_a.flat)
    if with_adam:
        for name in ("exp_avg", "exp_avg_sq", "step_count", "scalars"):
            getattr(opt_b, name).copy_(getattr(opt_a, name))
    ops.parameters_changed()
    return a, feed, b, x, y


@pytest.mark.parametrize("with_adam", [False, True])
def test_captured_training_fed_on_the_device_equals_set_batch(with_adam):
    from position_induced_transformer_amd import ops
    with ops.reproducible():
        a, feed, b, x, y = _train_pair(with_adam)
        assert feed.steps_per_epoch == 5 and int(feed.cursor) == 0   # the warm-up passes of capture() left the cursor alone
        seen = []
        for k in range(2 * feed.steps_per_epoch):
            a.replay()                                                # bare replays: no host data traffic
            idx, nv = feed.expected_indices(k)
            assert nv == 4
            pick = torch.tensor(idx, device="cuda")
            b.set_batch(x[pick], y[pick])
            b.replay()
            assert feed.indices.tolist() == idx, k
            assert _same_bits(a.func_in, x[pick]) and _same_bits(a.target, y[pick]), k
            assert _same_bits(a.func_in, b.func_in) and _same_bits(a.target, b.target), k
            assert _same_bits(a.loss, b.loss), (k, float(a.loss), float(b.loss))
            seen.append(idx)
        assert int(feed.cursor) == 10
        for epoch in (seen[:5], seen[5:]):
            assert sorted(j for idx in epoch for j in idx) == list(range(20))      # every sample once per epoch
        assert seen[:5] != seen[5:]
        pa = torch.cat([q.detach().reshape(-1) for q in a.model.parameters()])
        pb = torch.cat([q.detach().reshape(-1) for q in b.model.parameters()])
        assert torch.isfinite(pa).all() and _same_bits(pa, pb)
        if with_adam:
            assert int(a.optimizer.step_count) == int(b.optimizer.step_count)


def test_seek_and_capture_keep_the_cursor():
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    mesh, x, y = _fixed_data(20)
    step = TrainStep(_fixed_model(), (mesh, x[:4].clone(), mesh, y[:4].clone()), 1, 2)
    feed = DeviceFeed(step, {"func_in": x, "target": y}, seed=2)
    for k in (7, 0, 12):
        feed.seek(k)
        feed.launch()
        idx, _ = feed.expected_indices(k)
        assert feed.indices.tolist() == idx and int(feed.cursor) == k + 1
        assert _same_bits(step.func_in, x[torch.tensor(idx, device="cuda")])
    feed.seek(3)
    step.capture()                                                    # three warm-up passes, then the cursor is put back
    assert int(feed.cursor) == 3
    step.replay()
    assert feed.indices.tolist() == feed.expected_indices(3)[0] and int(feed.cursor) == 4
    step.run_eager()                                                  # the feed is the first launch of the eager step too
    assert feed.indices.tolist() == feed.expected_indices(4)[0] and int(feed.cursor) == 5
    with pytest.raises(RuntimeError, match="two sources"):
        step.set_batch(x[:4], y[:4])


def test_captured_evaluation_pass_fed_on_the_device():
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    ntest, batch = 21, 8
    mesh, x, y = _fixed_data(ntest, seed=22)
    with ops.reproducible():
        model = _fixed_model()
        fed = EvalStep(model, (mesh, x[:batch].clone(), mesh, y[:batch].clone()), 1, 2, capacity=ntest, store_pred=True)
        feed = DeviceFeed(fed, {"func_in": x, "target": y}, shuffle=False, drop_last=False)
        twin = EvalStep(model, (mesh, x[:batch].clone(), mesh, y[:batch].clone()), 1, 2, capacity=ntest, store_pred=True)
        fed.capture()
        twin.capture()
        assert feed.steps_per_epoch == 3
        twin.reset()
        for i in range(0, ntest, batch):
            twin.set_batch(x[i:i + batch], y[i:i + batch], n_valid=min(batch, ntest - i))
            twin.replay()
        want = twin.result()
        results = []
        for _ in range(2):                                            # a second pass after reset() gives the same
            fed.reset()
            for k in range(3):
                fed.replay()
                idx, nv = feed.expected_indices(k)
                assert feed.indices.tolist() == idx and int(fed.n_valid) == nv == min(batch, ntest - k * batch)
            got = fed.result()
            assert got.count == want.count == 21
            assert _same_bits(fed.per_sample, twin.per_sample) and _same_bits(fed.pred, twin.pred)
            for name in ("rel_lp", "rel_max", "worst_rel_lp", "worst_rel_max"):
                g_, w_ = getattr(got, name), getattr(want, name)
                assert abs(g_ - w_) <= 1e-12 * abs(w_), name
            results.append(got)
        assert results[0] == results[1]
        assert int(feed.cursor) == 3


def test_ragged_step_fed_on_the_device():
    """Clouds padded to 24 points: mesh, function, target and the int32 lengths all come through the one launch."""
    from position_induced_transformer_amd import ops, tasks
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    lengths = [24, 13, 19, 9, 24, 17, 11, 22, 15, 20]
    mesh, func, target, lens = tasks.ragged_clouds(lengths, 24, seed=31, device="cuda")
    with ops.reproducible():
        steps = []
        for fed in (True, False):
            torch.manual_seed(3)
            model = _freeze(tasks.pit_elasticity(2, 1, 1, 16, 2, 2, None, 0.2, 0.2).cuda())
            clouds = mesh[:3].clone()
            step = TrainStep(model, (clouds, func[:3].clone(), clouds, target[:3].clone()), 1, 2, len_in=lens[:3].clone())
            feed = DeviceFeed(step, {"mesh_in": mesh, "func_in": func, "target": target, "len_in": lens}, seed=4) if fed else None
            step.capture()
            steps.append((step, feed))
        (a, feed), (b, _) = steps
        assert feed.names == ["func_in", "target", "mesh_in", "len_in"] and feed.steps_per_epoch == 3
        for k in range(4):
            a.replay()
            idx, _ = feed.expected_indices(k)
            pick = torch.tensor(idx, device="cuda")
            b.set_batch(func[pick], target[pick], mesh_in=mesh[pick], len_in=lens[pick])
            b.replay()
            assert feed.indices.tolist() == idx
            assert _same_bits(a.mesh_in, mesh[pick]) and _same_bits(a.func_in, func[pick]) and _same_bits(a.target, target[pick])
            assert a.len_in.tolist() == [lengths[j] for j in idx]
            assert torch.isfinite(a.loss) and _same_bits(a.loss, b.loss), (k, float(a.loss), float(b.loss))


def test_rollout_step_fed_on_the_device():
    from position_induced_transformer_amd import ops, pit as P, tasks
    from position_induced_transformer_amd.engine import DeviceFeed, RolloutStep

    class _P2d(tasks._FixedMeshForward, P.pit_periodic2d):
        pass
    g = torch.Generator().manual_seed(41)
    n, batch, steps = 6, 2, 3
    mesh = tasks.grid_mesh_2d(8, False).cuda()
    x, y = torch.randn(n, 8, 8, 3, generator=g).cuda(), torch.randn(n, 8, 8, steps, generator=g).cuda()
    with ops.reproducible():
        pair = []
        for fed in (True, False):
            torch.manual_seed(3)
            model = _freeze(_P2d(2, 3, 1, 16, 2, 2, tasks.grid_mesh_2d(4, False).cuda(), 0.2, 0.2).cuda())
            step = RolloutStep(model, (mesh, x[:batch].clone(), y[:batch].clone()), steps, 1, 2)
            feed = DeviceFeed(step, {"func_in": x, "target": y}, seed=6) if fed else None
            step.capture()
            pair.append((step, feed))
        (a, feed), (b, _) = pair
        for k in range(2):
            a.replay()
            idx, _ = feed.expected_indices(k)
            pick = torch.tensor(idx, device="cuda")
            b.set_batch(x[pick], y[pick])
            b.replay()
            assert feed.indices.tolist() == idx
            assert _same_bits(a.func_in, x[pick]) and _same_bits(a.target, y[pick])
            assert torch.isfinite(a.loss) and _same_bits(a.loss, b.loss), (k, float(a.loss), float(b.loss))
        assert int(feed.cursor) == 2
