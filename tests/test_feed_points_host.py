"""No GPU: the subsampling feed entry (pit_batch_feed_points) in header, binding and source, its refusals before any launch in
their documented order, the host restatement of the point subsets (engine.feed_points) with the uniformity of inclusion, and
the host-side checks of engine.DeviceFeed(subsample=True)."""
import ctypes
import math
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h
C1, C2, M64 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, (1 << 64) - 1


# ----------------------------------------------------------------------------- header, binding, source
def test_header_binding_and_source_agree_on_the_points_entry():
    from position_induced_transformer_amd import _lib, build
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_FEED_POINTS 1$", text, flags=re.M)
    assert re.search(r"^#define PIT_HAS_BATCH_FEED 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    for name, value in (("WHOLE_ROW", 0), ("POINTS_G0", 1), ("POINTS_G1", 2)):
        assert int(re.search(rf"^#define PIT_FEED_{name} (\d+)$", text, flags=re.M).group(1)) == getattr(_lib, "FEED_" + name) == value
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "pit_batch_feed_points"
    assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]) == 27
    assert hasattr(_lib.lib(), name) and _lib.lib().pit_version() == 31
    assert len(_lib.SIGNATURES["pit_batch_feed"]) == 16               # the plain entry is as it was
    block = text[text.index("A random subset of each cloud's points"):text.index("#define PIT_HAS_FEED_POINTS")]
    assert "train_elasticity.py:64,86-88" in block and "0x9E3779B97F4A7C15" in block and "0xD1B54A32D192ED03" in block
    src = open(os.path.join(build.CSRC, "pit_feed.hip")).read()
    assert "batch_feed_points_kernel" in src and "batch_feed_kernel" in src
    assert "re-enters [0, n)" in src                                  # why the cycle walk ends, noted where it runs


# ----------------------------------------------------------------------------- refusals before any launch
_buf = (ctypes.c_longlong * 64)()
P = ctypes.addressof(_buf)
A = ctypes.addressof


def _ptrs(**changed):
    a = (ctypes.c_void_p * 8)(*[P] * 8)
    for i, v in changed.items():
        a[int(i[1:])] = v
    return A(a), a                                                    # (the array is kept alive by the caller's tuple)


def _longs(*values):
    a = (ctypes.c_long * 8)(*(list(values) + [4] * (8 - len(values))))
    return A(a), a


def _ints(*values):
    a = (ctypes.c_int * 8)(*(list(values) + [0] * (8 - len(values))))
    return A(a), a


_SRC, _DST = _ptrs(), _ptrs()
_BYTES = _longs(8, 4, 176, 12, 64)
_KIND = _ints(1, 1, 2, 2, 0)
BASE = dict(src=_SRC[0], dst=_DST[0], bytes=_BYTES[0], kind=_KIND[0], n_fields=5, n0=972, m0=486, n1=100, m1=100,
            len_src0=P, len_src1=None, len_dst0=P, len_dst1=P, points0=P, points1=None,
            n_samples=37, batch=8, rank=1, world=2, drop_last=1, shuffle=1, order=None, seed=7, state=P, indices=None,
            n_valid=None, stream=None)

_KEEP = [_ptrs(_0=None), _ptrs(_4=None), _ptrs(_5=None), _ints(1, 1, 2, 3, 0), _ints(1, 1, 2, -1, 0), _longs(0), _longs(8, 6),
         _longs(8, 4, 176, 12, -4), _ptrs(_1=P + 2), _ptrs(_3=P + 1), _ints(0, 0, 2, 2, 0), _ints(1, 1, 0, 0, 0),
         _longs(8, 4, (1 << 30) // 100 // 4 * 4 + 4), _longs(8, 4, 176, 12, (1 << 30) + 4), None,
         _longs(8, 4, (1 << 30) // 100 // 4 * 4 + 4, 12, 6), _longs((1 << 30) // 972 // 4 * 4 + 4)]

TABLE = [                                                             # in the header's order
    (dict(src=None), NULL),
    (dict(dst=None), NULL),
    (dict(bytes=None), NULL),
    (dict(kind=None), NULL),
    (dict(state=None), NULL),
    (dict(n_fields=0), SIZE),
    (dict(n_fields=-1), SIZE),
    (dict(n_fields=9), SIZE),
    (dict(n_fields=9, src=_KEEP[0][0]), SIZE),                        # (the count is looked at before the entries)
    (dict(src=_KEEP[0][0]), NULL),                                    # a null entry among the fields in use
    (dict(dst=_KEEP[1][0]), NULL),
    (dict(src=_KEEP[0][0], n_samples=0), NULL),                       # (null entries before the sizes)
    (dict(n_samples=0), SIZE),
    (dict(n_samples=-5), SIZE),
    (dict(batch=0), SIZE),
    (dict(batch=-1), SIZE),
    (dict(batch=65536), SIZE),                                        # the grid limit
    (dict(world=0), SIZE),
    (dict(world=-2), SIZE),
    (dict(rank=-1), SIZE),
    (dict(rank=2), SIZE),
    (dict(drop_last=2), SIZE),
    (dict(drop_last=-1), SIZE),
    (dict(shuffle=2), SIZE),
    (dict(shuffle=-1), SIZE),
    (dict(kind=_KEEP[3][0]), SIZE),                                   # kind 3
    (dict(kind=_KEEP[4][0]), SIZE),                                   # kind -1
    (dict(bytes=_KEEP[5][0]), SIZE),                                  # a point of 0 bytes
    (dict(bytes=_KEEP[6][0]), SIZE),                                  # 6: no multiple of 4
    (dict(bytes=_KEEP[7][0]), SIZE),                                  # negative
    (dict(src=_KEEP[8][0]), SIZE),                                    # a pointer off a 4-byte boundary
    (dict(dst=_KEEP[9][0]), SIZE),
    (dict(n1=0, m1=0, len_dst1=None), SIZE),                          # point fields of group 1, which has no widths
    (dict(n0=0, m0=0), SIZE),
    (dict(m0=0), SIZE),                                               # m_g < 1
    (dict(m0=-3), SIZE),
    (dict(m0=973), SIZE),                                             # m_g > n_g
    (dict(m1=101), SIZE),
    (dict(len_src0=P + 2), SIZE),                                     # lengths and tables are int32 arrays
    (dict(len_dst1=P + 1), SIZE),
    (dict(points0=P + 3), SIZE),
    (dict(kind=_KEEP[10][0]), SIZE),                                  # no field of group 0, but its lengths and table are given
    (dict(kind=_KEEP[11][0]), SIZE),                                  # no field of group 1, but len_dst1 is given
    (dict(n_samples=15), SIZE),                                       # drop_last and fewer samples than one step of all ranks
    (dict(n_samples=1 << 31), UNSUPPORTED),
    (dict(n_samples=1 << 40, drop_last=0), UNSUPPORTED),
    (dict(bytes=_KEEP[12][0]), UNSUPPORTED),                          # n_1 = 100 points of this size pass 1 GiB
    (dict(bytes=_KEEP[13][0]), UNSUPPORTED),                          # a whole row beyond PIT_FEED_MAX_ROW_BYTES
    (dict(bytes=_KEEP[16][0]), UNSUPPORTED),                          # n_0 = 972 points
    (dict(bytes=_KEEP[15][0]), SIZE),                                 # (the size refusals come first)
    (dict(bytes=_KEEP[12][0], n_samples=15), SIZE),
]


def test_batch_feed_points_refuses_bad_arguments_in_the_documented_order():
    from position_induced_transformer_amd import _lib
    fn = _lib.lib().pit_batch_feed_points
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\bpit_batch_feed_points\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert [re.split(r"[\s*]+", a.strip())[-1] for a in args.split(",")] == list(BASE)    # the table's argument order is the header's
    for changed, want in TABLE:
        assert set(changed) <= set(BASE)
        assert fn(*{**BASE, **changed}.values()) == want, changed
    # a null entry BEYOND n_fields is not looked at: refused for nothing but the size that follows
    assert fn(*{**BASE, "src": _KEEP[2][0], "n_samples": 0}.values()) == SIZE
    # a group without fields and without pointers may carry any widths
    assert fn(*{**BASE, "kind": _KEEP[11][0], "len_dst1": None, "n1": 0, "m1": 5, "n_samples": 1 << 31}.values()) == UNSUPPORTED


def test_ops_batch_feed_points_refuses_host_tensors_and_misfits():
    from position_induced_transformer_amd import ops
    src, dst, state = torch.zeros(5, 6, 3), torch.zeros(2, 4, 3), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.batch_feed_points([src], [dst], [1], state)
    with pytest.raises(ValueError, match="fields"):
        ops.batch_feed_points([], [], [], state)
    with pytest.raises(ValueError, match="fields"):
        ops.batch_feed_points([src], [dst], [1, 1], state)
    with pytest.raises(ValueError, match="per group"):
        ops.batch_feed_points([src], [dst], [1], state, points=(None,))


# ----------------------------------------------------------------------------- engine.feed_points
@pytest.mark.parametrize("L", [1, 2, 3, 5, 16, 17, 65, 1000])
def test_feed_points_is_the_head_of_the_keyed_permutation(L):
    from position_induced_transformer_amd.engine import feed_order, feed_points
    seed = (5 << 32) | 9
    for m in sorted({1, max(L - 1, 1), L, L + 3}):
        for epoch, sample, group in ((0, 0, 0), (3, 7, 1), (1, 2 ** 31 - 2, 0)):
            a = feed_points(L, m, seed, epoch, sample, group)
            assert a.dtype == torch.int64 and a.device.type == "cpu" and a.shape == (min(m, L),)
            assert len(set(a.tolist())) == a.numel() and 0 <= int(a.min()) and int(a.max()) < L
            key = (seed ^ (((sample + 1) * C1 + group * C2) & M64)) & M64
            assert torch.equal(a, feed_order(L, key, epoch)[:m])
            assert torch.equal(a, feed_points(L, m, seed, epoch, sample, group))      # reproducible
            if m >= L:
                assert sorted(a.tolist()) == list(range(L))          # the whole cloud, permuted
    assert feed_points(L, 4, seed, 0, 3).tolist() == feed_points(L, 4, seed, 0, 3, group=0).tolist()
    if L >= 5:                                                        # (L = 2, 3 have too few permutations to ask for it)
        base = feed_points(L, L, seed, 0, 3, 0).tolist()
        assert base != feed_points(L, L, seed, 0, 3, 1).tolist()      # the other group
        assert base != feed_points(L, L, seed, 0, 4, 0).tolist()      # another sample
        assert base != feed_points(L, L, seed, 1, 3, 0).tolist()      # another epoch
        assert base != feed_points(L, L, seed + 1, 0, 3, 0).tolist()  # another seed
    for bad in (dict(length=0), dict(m=0), dict(sample=-1), dict(group=2)):
        with pytest.raises(ValueError):
            feed_points(**{**dict(length=5, m=2, seed=0, epoch=0, sample=0, group=0), **bad})


@pytest.mark.parametrize("L,m,epochs", [(5, 2, 4000), (17, 4, 4000), (65, 16, 4000), (257, 64, 4000), (1000, 250, 2000),
                                        (4097, 512, 1000)])
def test_every_point_is_included_equally_often(L, m, epochs):
    """Over E epochs a point's inclusion count is Binomial(E, p = m / L) under a uniform subset: every count must lie within 5
    standard deviations sqrt(E p (1 - p)) of E p.  A condition on the permutation rule (measured on it: 3.73 at worst over
    these shapes), not a tuned number."""
    from position_induced_transformer_amd.engine import feed_points
    p = m / L
    sd = math.sqrt(epochs * p * (1 - p))
    for sample in (0, 7):
        count = torch.zeros(L, dtype=torch.int64)
        for e in range(epochs):
            count[feed_points(L, m, 5, e, sample)] += 1
        worst = float((count.double() - epochs * p).abs().max()) / sd
        print(f"L {L} m {m} epochs {epochs} sample {sample}: worst deviation {worst:.2f} sd")
        assert worst <= 5.0, (sample, worst)


# ----------------------------------------------------------------------------- engine.DeviceFeed(subsample=True) on CPU steps
def _model(batched=True):
    from position_induced_transformer_amd import pit as P_, tasks
    torch.manual_seed(0)
    if batched:                                                       # per-sample clouds; forward takes len_in / len_out
        return tasks.pit_elasticity(2, 1, 1, 16, 2, 1, None, 0.1, 0.1)
    return P_.pit_fixed(2, 1, 1, 16, 2, 4, torch.rand(16, 2), 0.1, 0.1)


def _batch(b=4, m=8, one_cloud=False):
    mesh = torch.zeros(b, m, 2)
    return mesh, torch.zeros(b, m, 1), (mesh if one_cloud else torch.zeros(b, m, 2)), torch.zeros(b, m, 1)


def _eval(b=4, m=8, one_cloud=False, batched=True, **kw):
    from position_induced_transformer_amd.engine import EvalStep
    return EvalStep(_model(batched), _batch(b, m, one_cloud), 1, 2, **kw)


def _data(N=13, n=20, one_cloud=False, **extra):
    mesh = torch.rand(N, n, 2)
    d = {"mesh_in": mesh, "func_in": torch.rand(N, n, 1), "mesh_out": mesh if one_cloud else torch.rand(N, n, 2),
         "target": torch.rand(N, n, 1)}
    d.update(extra)
    return d


def _lens(N=13, lo=8, hi=20, seed=1):
    return torch.randint(lo, hi + 1, (N,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def test_subsample_feed_attributes_and_groups():
    from position_induced_transformer_amd.engine import DeviceFeed
    step = _eval()
    feed = DeviceFeed(step, _data(), seed=5, subsample=True)
    assert step._feed is feed and feed.subsample and feed.names == ["func_in", "target", "mesh_in", "mesh_out"]
    assert feed.kinds == [1, 2, 1, 2] and (feed.n_in, feed.m_in, feed.n_out, feed.m_out) == (20, 8, 20, 8)
    for t in (feed.points_in, feed.points_out):
        assert t.dtype == torch.int32 and t.shape == (4, 8)
    one = DeviceFeed(_eval(one_cloud=True), _data(one_cloud=True), subsample=True)
    assert one.kinds == [1, 1, 1] and one.names == ["func_in", "target", "mesh_in"]      # target follows the one cloud
    assert one.points_out is None and (one.n_out, one.m_out) == (0, 0)
    plain = DeviceFeed(_eval(m=20), _data())
    assert not plain.subsample and plain.points_in is None and plain.points_out is None
    with pytest.raises(ValueError, match="without subsample"):
        plain.expected_points(0)


def test_subsample_refusals_before_any_launch():
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep
    data = _data()
    # a point field whose cloud's mesh is not in data
    for missing, field in (("mesh_in", "func_in"), ("mesh_out", "target")):
        with pytest.raises(ValueError, match=f"point field {field} without {missing}"):
            DeviceFeed(_eval(), {k: v for k, v in data.items() if k != missing}, subsample=True)
    with pytest.raises(ValueError, match="point field target without mesh_in"):
        DeviceFeed(_eval(one_cloud=True), {"target": data["target"]}, subsample=True)
    # a batch-free model: its mesh plans were built once
    with pytest.raises(ValueError, match="batch-free"):
        DeviceFeed(_eval(batched=False), data, subsample=True)
    # pred_affine, store_pred
    affine = (torch.ones(8, 1), torch.zeros(8, 1))
    with pytest.raises(ValueError, match="pred_affine"):
        DeviceFeed(EvalStep(_model(), _batch(), 1, 2, pred_affine=affine), data, subsample=True)
    with pytest.raises(ValueError, match="store_pred"):
        DeviceFeed(_eval(capacity=13, store_pred=True), data, subsample=True)
    # data narrower than the step; clouds whose fields disagree; other trailing shapes and dtypes
    with pytest.raises(ValueError, match="narrower than the step"):
        DeviceFeed(_eval(m=21), data, subsample=True)
    with pytest.raises(ValueError, match="fields of its cloud"):
        DeviceFeed(_eval(), {**data, "func_in": torch.rand(13, 19, 1)}, subsample=True)
    with pytest.raises(ValueError, match="points"):
        DeviceFeed(_eval(), {**data, "target": torch.rand(13, 20, 2)}, subsample=True)
    with pytest.raises(ValueError, match="points"):
        DeviceFeed(_eval(), {**data, "target": torch.rand(13, 20, 1, dtype=torch.float64)}, subsample=True)
    with pytest.raises(ValueError, match="samples"):
        DeviceFeed(_eval(), {**data, "target": torch.rand(12, 20, 1)}, subsample=True)
    # lengths
    with pytest.raises(ValueError, match="integer lengths"):
        DeviceFeed(_eval(), {**data, "len_in": torch.ones(12, dtype=torch.int32)}, subsample=True)
    with pytest.raises(ValueError, match="one length"):
        DeviceFeed(_eval(one_cloud=True), _data(one_cloud=True, len_out=_lens()), subsample=True)
    with pytest.raises(ValueError, match="lengths only"):
        DeviceFeed(_eval(), {"len_in": _lens()}, subsample=True)
    step = _eval()
    with pytest.raises(ValueError, match="narrower"):
        DeviceFeed(step, _data(n=7), subsample=True)
    assert step._feed is None                                         # a refused feed is not attached
    # without subsample everything is as it was: the rows must match, lengths need a step with lengths
    with pytest.raises(ValueError, match="rows"):
        DeviceFeed(_eval(), data)
    with pytest.raises(ValueError, match="built without len_in"):
        DeviceFeed(_eval(m=20), {**data, "len_in": _lens()})


def test_the_shortest_cloud_must_fill_a_step_without_lengths():
    from position_induced_transformer_amd.engine import DeviceFeed
    lens = _lens(lo=8)
    lens[5] = 6
    with pytest.raises(ValueError, match=r"shortest cloud of len_in has 6 points, the step takes 8; build the step with len_in="):
        DeviceFeed(_eval(), _data(len_in=lens), subsample=True)
    with pytest.raises(ValueError, match=r"shortest cloud of len_out has 6 points.*len_out="):
        DeviceFeed(_eval(), _data(len_out=lens), subsample=True)
    lens[5] = 8
    feed = DeviceFeed(_eval(), _data(len_in=lens, len_out=lens.to(torch.int64)), subsample=True)
    assert feed._len_dst == [None, None] and feed._len_src[0].tolist() == lens.tolist() and feed._len_src[1].dtype == torch.int32
    # a step WITH lengths takes any cloud: the launch then writes min(m, length)
    lens[5] = 2
    step = _eval(len_in=[8] * 4)
    feed = DeviceFeed(step, _data(len_in=lens), subsample=True)
    assert feed._len_dst[0] is step.len_in and feed._len_dst[1] is None
    # ... and a step with lengths fed from data without: the launch writes m
    feed = DeviceFeed(_eval(len_in=[8] * 4, len_out=[8] * 4), _data(), subsample=True)
    assert feed._len_src == [None, None] and all(t is not None for t in feed._len_dst)


def test_state_dict_keys_with_and_without_subsample():
    from position_induced_transformer_amd.engine import DeviceFeed
    plain = DeviceFeed(_eval(m=20), _data(), seed=5)
    plain.seek(3)
    assert plain.state_dict() == {"cursor": 3, "n_samples": 13, "batch": 4, "world_size": 1, "seed": 5, "shuffle": True,
                                  "drop_last": True, "steps_per_epoch": 3}      # exactly the dict of a feed before subsets
    feed = DeviceFeed(_eval(), _data(), seed=5, subsample=True)
    feed.seek(7)
    state = feed.state_dict()
    assert state == {**plain.state_dict(), "cursor": 7, "subsample": True, "n_in": 20, "m_in": 8, "n_out": 20, "m_out": 8}
    other = DeviceFeed(_eval(), _data(), seed=5, subsample=True)
    other.load_state_dict(state)
    assert int(other.cursor) == 7
    with pytest.raises(ValueError, match="subsample"):
        plain.load_state_dict(state)
    with pytest.raises(ValueError, match="subsample"):
        other.load_state_dict(plain.state_dict())
    for key, value in (("n_in", 21), ("m_in", 7), ("n_out", 19), ("m_out", 4), ("seed", 6)):
        with pytest.raises(ValueError, match=key):
            other.load_state_dict({**state, key: value})
    narrower = DeviceFeed(_eval(m=6), _data(), seed=5, subsample=True)
    with pytest.raises(ValueError, match="m_in"):
        narrower.load_state_dict(state)
    assert int(narrower.cursor) == 0


def test_expected_points_restate_feed_points():
    from position_induced_transformer_amd.engine import DeviceFeed, feed_points
    lens_in, lens_out = _lens(lo=1, seed=1), _lens(lo=1, seed=2)
    lens_in[0], lens_out[1] = 0, 99                                   # clamped into [1, n] where they are read
    step = _eval(len_in=[8] * 4, len_out=[8] * 4)
    feed = DeviceFeed(step, _data(len_in=lens_in, len_out=lens_out), seed=11, subsample=True)
    for cursor in (0, 1, 2, 3, 7):
        idx, _ = feed.expected_indices(cursor)
        epoch = cursor // feed.steps_per_epoch
        pin, pout = feed.expected_points(cursor)
        assert len(pin) == len(pout) == 4
        for s, i in enumerate(idx):
            L0, L1 = min(max(int(lens_in[i]), 1), 20), min(max(int(lens_out[i]), 1), 20)
            assert torch.equal(pin[s], feed_points(L0, 8, 11, epoch, i, 0)) and pin[s].numel() == min(8, L0)
            assert torch.equal(pout[s], feed_points(L1, 8, 11, epoch, i, 1)) and pout[s].numel() == min(8, L1)
    nolen = DeviceFeed(_eval(one_cloud=True), _data(one_cloud=True), seed=11, subsample=True)
    pin, pout = nolen.expected_points(4)
    assert pout is None and all(torch.equal(q, feed_points(20, 8, 11, 1, i, 0)) for q, i in zip(pin, nolen.expected_indices(4)[0]))


def test_two_ranks_hold_disjoint_samples_and_the_same_subset_per_sample():
    from position_induced_transformer_amd.engine import DeviceFeed
    N, world = 16, 2
    data = _data(N=N)
    feeds = [DeviceFeed(_eval(), data, seed=3, rank=r, world_size=world, subsample=True) for r in range(world)]
    alone = DeviceFeed(_eval(), data, seed=3, rank=0, world_size=1, subsample=True)
    assert feeds[0].steps_per_epoch == 2 and alone.steps_per_epoch == 4
    for epoch in (0, 1):
        subset = {}
        for i in range(4):                                            # a sample's subset as the single-rank run draws it
            for s, j in enumerate(alone.expected_indices(epoch * 4 + i)[0]):
                pts = alone.expected_points(epoch * 4 + i)
                subset[j] = (pts[0][s], pts[1][s])
        assert len(subset) == N
        seen = []
        for i in range(2):
            for f in feeds:
                idx, _ = f.expected_indices(epoch * 2 + i)
                pin, pout = f.expected_points(epoch * 2 + i)
                seen += idx
                for s, j in enumerate(idx):
                    assert torch.equal(pin[s], subset[j][0]) and torch.equal(pout[s], subset[j][1])
        assert sorted(seen) == list(range(N))                         # disjoint across the ranks, together the epoch
