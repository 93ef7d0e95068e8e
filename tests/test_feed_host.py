"""No GPU: the data-feed entry (pit_batch_feed) in header, binding and source list, its refusals before any launch, the host
restatement of the keyed permutation (engine.feed_order), the sharding engine.DeviceFeed.expected_indices describes, and the
host-side checks of engine.DeviceFeed."""
import ctypes
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pit_hip.h")

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                  # PIT_ERR_* of include/pit_hip.h


# ----------------------------------------------------------------------------- header, binding, sources
def test_header_binding_and_sources_agree_on_the_feed_entry():
    from position_induced_transformer_amd import _lib, build
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_BATCH_FEED 1$", text, flags=re.M)
    assert int(re.search(r"^#define PIT_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _lib.ABI_VERSION == 31
    assert int(re.search(r"^#define PIT_FEED_MAX_FIELDS (\d+)$", text, flags=re.M).group(1)) == _lib.FEED_MAX_FIELDS == 8
    assert re.search(r"^#define PIT_FEED_MAX_ROW_BYTES \(1L << 30\)$", text, flags=re.M) and _lib.FEED_MAX_ROW_BYTES == 1 << 30
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "pit_batch_feed"
    assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]) == 16
    assert hasattr(_lib.lib(), name)
    assert "pit_feed.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pit_feed.hip"))
    assert _lib.lib().pit_version() == 31
    assert "train_darcy.py:98,124-126" in text[text.index("pit_feed.hip"):text.index("#define PIT_HAS_BATCH_FEED")]


# ----------------------------------------------------------------------------- refusals before any launch
_buf = (ctypes.c_longlong * 64)()
P = ctypes.addressof(_buf)
_SRC, _DST = (ctypes.c_void_p * 8)(*[P] * 8), (ctypes.c_void_p * 8)(*[P] * 8)
_ROWS = (ctypes.c_long * 8)(4, 12, 16, 7396, 65540, 8, 4, 4)


def _ptrs(**changed):
    a = (ctypes.c_void_p * 8)(*[P] * 8)
    for i, v in changed.items():
        a[int(i[1:])] = v
    return ctypes.addressof(a), a                                     # (the array is kept alive by the caller's tuple)


def _rows(*values):
    a = (ctypes.c_long * 8)(*(list(values) + [4] * (8 - len(values))))
    return ctypes.addressof(a), a


A = ctypes.addressof
BASE = dict(src=A(_SRC), dst=A(_DST), row_bytes=A(_ROWS), n_fields=5, n_samples=37, batch=8, rank=1, world=2, drop_last=1,
            shuffle=1, order=None, seed=7, state=P, indices=None, n_valid=None, stream=None)

_KEEP = [_ptrs(_0=None), _ptrs(_4=None), _ptrs(_5=None), _rows(0), _rows(4, 6), _rows(4, 12, 16, 7396, -4), _rows(4, 12, 16, 7396, 2),
         _ptrs(_1=P + 2), _ptrs(_3=P + 1), _rows(4, 12, (1 << 30) + 4), _rows(4, 12, 1 << 30, 7396, 6)]

TABLE = [
    (dict(src=None), NULL),
    (dict(dst=None), NULL),
    (dict(row_bytes=None), NULL),
    (dict(state=None), NULL),
    (dict(src=_KEEP[0][0]), NULL),                                    # a null entry among the fields in use
    (dict(dst=_KEEP[1][0]), NULL),
    (dict(n_fields=0), SIZE),
    (dict(n_fields=-1), SIZE),
    (dict(n_fields=9), SIZE),
    (dict(n_samples=0), SIZE),
    (dict(n_samples=-5), SIZE),
    (dict(batch=0), SIZE),
    (dict(batch=-1), SIZE),
    (dict(batch=65536), SIZE),                                        # the grid limit
    (dict(world=0), SIZE),
    (dict(world=-2), SIZE),
    (dict(rank=-1), SIZE),
    (dict(rank=2), SIZE),
    (dict(row_bytes=_KEEP[3][0]), SIZE),                              # a row of 0 bytes
    (dict(row_bytes=_KEEP[4][0]), SIZE),                              # 6: no multiple of 4
    (dict(row_bytes=_KEEP[5][0]), SIZE),                              # negative
    (dict(row_bytes=_KEEP[6][0]), SIZE),
    (dict(src=_KEEP[7][0]), SIZE),                                    # rows move as aligned words: a pointer off a 4-byte boundary
    (dict(dst=_KEEP[8][0]), SIZE),
    (dict(n_samples=15), SIZE),                                       # drop_last and fewer samples than one step of all ranks
    (dict(drop_last=2), SIZE),
    (dict(drop_last=-1), SIZE),
    (dict(shuffle=2), SIZE),
    (dict(shuffle=-1), SIZE),
    (dict(n_samples=1 << 31), UNSUPPORTED),
    (dict(n_samples=1 << 40, drop_last=0), UNSUPPORTED),
    (dict(row_bytes=_KEEP[9][0]), UNSUPPORTED),                       # a row beyond PIT_FEED_MAX_ROW_BYTES (1 GiB exactly is taken)
    (dict(row_bytes=_KEEP[10][0]), SIZE),                             # (the size refusals come first)
]


def test_batch_feed_refuses_bad_arguments_before_any_launch():
    from position_induced_transformer_amd import _lib
    fn = _lib.lib().pit_batch_feed
    assert list(BASE) == ["src", "dst", "row_bytes", "n_fields", "n_samples", "batch", "rank", "world", "drop_last", "shuffle",
                          "order", "seed", "state", "indices", "n_valid", "stream"]
    assert len(BASE) == len(_lib.SIGNATURES["pit_batch_feed"])       # the table's argument order is the header's
    for changed, code in TABLE:
        assert set(changed) <= set(BASE)
        assert fn(*{**BASE, **changed}.values()) == code, changed
    # a null entry BEYOND n_fields is not looked at: the call above with the sixth entry missing is refused for nothing else
    assert fn(*{**BASE, "src": _KEEP[2][0], "n_samples": 0}.values()) == SIZE


def test_ops_batch_feed_refuses_host_tensors_and_misfits():
    from position_induced_transformer_amd import ops
    src, dst, state = torch.zeros(5, 3), torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.batch_feed([src], [dst], state)
    with pytest.raises(ValueError, match="fields"):
        ops.batch_feed([], [], state)
    with pytest.raises(ValueError, match="fields"):
        ops.batch_feed([src] * 9, [dst] * 9, state)


# ----------------------------------------------------------------------------- the keyed permutation
SIZES = (1, 2, 3, 5, 16, 17, 37, 1000, 1024, 1025)


def _fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _scalar_order(n, seed, epoch):
    """The header's pseudo-code, one position at a time in Python integers."""
    bits = max(2, (n - 1).bit_length())
    bits += bits & 1
    half = bits // 2
    mask = (1 << half) - 1
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    key = [_fmix(lo ^ _fmix((hi + 0x9E3779B9 * (epoch + 1) + j) & 0xFFFFFFFF)) for j in range(4)]
    out = []
    for g in range(n):
        x = g
        while True:
            left, right = x >> half, x & mask
            for j in range(4):
                left, right = right, left ^ (_fmix((right + key[j]) & 0xFFFFFFFF) & mask)
            x = (left << half) | right
            if x < n:
                break
        out.append(x)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_feed_order_is_a_keyed_permutation(n):
    from position_induced_transformer_amd.engine import feed_order
    a = feed_order(n, 3, 0)
    assert a.dtype == torch.int64 and a.device.type == "cpu" and a.shape == (n,)
    for seed, epoch in ((3, 0), (3, 1), (4, 0), ((5 << 32) | 9, 7), (3, (1 << 32) + 1)):
        o = feed_order(n, seed, epoch)
        assert sorted(o.tolist()) == list(range(n)), (seed, epoch)
        assert torch.equal(o, feed_order(n, seed, epoch))            # reproducible
    assert torch.equal(feed_order(n, 3, (1 << 32) + 1), feed_order(n, 3, 1))      # the epoch counts mod 2^32
    if n <= 1025:
        assert a.tolist() == _scalar_order(n, 3, 0)
        assert feed_order(n, (5 << 32) | 9, 7).tolist() == _scalar_order(n, (5 << 32) | 9, 7)
    if n >= 3:
        assert not torch.equal(a, feed_order(n, 3, 1))
        assert not torch.equal(a, feed_order(n, 4, 0))
    a[0] = -1                                                         # the caller's copy: the next call is not affected
    assert feed_order(n, 3, 0)[0] >= 0


# ----------------------------------------------------------------------------- engine.DeviceFeed on CPU tensors
def _cpu_model():
    from position_induced_transformer_amd import pit as P_
    torch.manual_seed(0)
    return P_.pit_fixed(2, 1, 1, 16, 2, 4, torch.rand(16, 2), 0.1, 0.1)


def _cpu_batch(b=8, n=36):
    x = torch.zeros(b, n, 1)
    return torch.rand(n, 2), x, torch.rand(n, 2), x.clone()


def _eval_step(b=8, **kw):
    from position_induced_transformer_amd.engine import EvalStep
    return EvalStep(_cpu_model(), _cpu_batch(b), 1, 2, **kw)


def _data(n=37, pts=36):
    return {"func_in": torch.rand(n, pts, 1), "target": torch.rand(n, pts, 1)}


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("drop_last", [True, False])
def test_expected_indices_shard_an_epoch(world, drop_last):
    from position_induced_transformer_amd.engine import DeviceFeed, feed_order
    n, batch = 37, 8
    feeds = [DeviceFeed(_eval_step(batch), _data(n), seed=11, drop_last=drop_last, rank=r, world_size=world) for r in range(world)]
    steps = n // (batch * world) if drop_last else -(-n // (batch * world))
    assert all(f.steps_per_epoch == steps for f in feeds)
    for epoch in (0, 1):
        order = feed_order(n, 11, epoch).tolist()
        seen, valid = [], 0
        for i in range(steps):
            for f in feeds:                                           # the ranks of one step, in rank order
                idx, nv = f.expected_indices(epoch * steps + i)
                assert len(idx) == batch and all(0 <= j < n for j in idx)
                if drop_last:
                    assert nv == batch
                seen += idx[:nv]
                valid += nv
                first = (i * world + f.rank) * batch
                assert idx == [order[(first + s) % n] for s in range(batch)]      # past the end the positions wrap
        if drop_last:
            assert len(set(seen)) == len(seen) == steps * batch * world
            assert seen == order[:steps * batch * world]
        else:
            assert valid == n and seen == order
    assert feeds[0].expected_indices(0)[0] != feeds[0].expected_indices(steps)[0]  # the next epoch has another order


def test_expected_indices_identity_and_caller_order():
    from position_induced_transformer_amd.engine import DeviceFeed
    f = DeviceFeed(_eval_step(8), _data(37), shuffle=False, drop_last=False, rank=1, world_size=2)
    assert f.steps_per_epoch == 3
    assert f.expected_indices(0) == (list(range(8, 16)), 8)
    assert f.expected_indices(2) == ([3, 4, 5, 6, 7, 8, 9, 10], 0)   # (2*2 + 1)*8 = 40 > 37: wrapped, none valid
    assert f.expected_indices(5) == f.expected_indices(2)            # the identity does not depend on the epoch
    order = torch.arange(36, -1, -1)
    order[3], order[4] = -7, 1 << 40                                  # clamped where they are read
    g = DeviceFeed(_eval_step(8), _data(37), order=order, drop_last=False)
    assert g.order.dtype == torch.int32 and g.order.shape == (37,)
    assert g.expected_indices(0) == ([36, 35, 34, 0, 36, 31, 30, 29], 8)
    assert g.expected_indices(4) == ([4, 3, 2, 1, 0, 36, 35, 34], 5)


def test_device_feed_constructor_checks():
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep, RolloutStep, TrainStep
    step = _eval_step(8)
    feed = DeviceFeed(step, _data(), seed=5)
    assert step._feed is feed and feed.steps_per_epoch == 4 and feed.rank == 0 and feed.world_size == 1
    assert feed.cursor.dtype == torch.int64 and int(feed.cursor) == 0
    assert feed.indices.dtype == torch.int32 and feed.indices.shape == (8,) and feed.order is None
    feed.seek(9)
    assert int(feed.cursor) == 9 and feed.state.tolist() == [9, 0]
    with pytest.raises(ValueError, match="already has a feed"):
        DeviceFeed(step, _data())
    with pytest.raises(ValueError, match="unknown field"):
        DeviceFeed(_eval_step(), {**_data(), "labels": torch.zeros(37)})
    with pytest.raises(ValueError, match="batch-free"):              # pit_fixed: the mesh plans were built once
        DeviceFeed(_eval_step(), {**_data(), "mesh_in": torch.rand(37, 36, 2)})
    with pytest.raises(ValueError, match="batch-free"):
        DeviceFeed(_eval_step(), {**_data(), "mesh_out": torch.rand(37, 36, 2)})
    for name in ("len_in", "len_out"):
        with pytest.raises(ValueError, match=f"built without {name}"):
            DeviceFeed(_eval_step(), {**_data(), name: torch.ones(37, dtype=torch.int32)})
    # rows, dtypes, sample counts, contiguity
    with pytest.raises(ValueError, match="rows"):
        DeviceFeed(_eval_step(), {**_data(), "target": torch.rand(37, 35, 1)})
    with pytest.raises(ValueError, match="rows"):
        DeviceFeed(_eval_step(), {**_data(), "target": torch.rand(37, 36, 1, dtype=torch.float64)})
    with pytest.raises(ValueError, match="samples"):
        DeviceFeed(_eval_step(), {**_data(), "target": torch.rand(36, 36, 1)})
    with pytest.raises(ValueError, match="contiguous"):
        DeviceFeed(_eval_step(), {**_data(), "target": torch.rand(37, 36, 2)[..., :1]})
    with pytest.raises(ValueError, match="no full step"):
        DeviceFeed(_eval_step(), _data(7))
    with pytest.raises(ValueError, match="rank"):
        DeviceFeed(_eval_step(), _data(), rank=2, world_size=2)
    with pytest.raises(ValueError, match="order"):
        DeviceFeed(_eval_step(), _data(), order=torch.arange(36))
    # the training steps have no n_valid: a partly filled batch would enter the loss
    model = _cpu_model()
    mesh, x, _, y = _cpu_batch()
    train = TrainStep(model, (mesh, x, mesh, y), 1, 2)
    with pytest.raises(ValueError, match="drop_last=False on a TrainStep"):
        DeviceFeed(train, _data(), drop_last=False)
    roll = RolloutStep(model, (mesh, x, torch.zeros(8, 36, 3)), 3, 1, 2)
    with pytest.raises(ValueError, match="drop_last=False on a RolloutStep"):
        DeviceFeed(roll, {"func_in": torch.rand(37, 36, 1), "target": torch.rand(37, 36, 3)}, drop_last=False)
    assert train._feed is None and roll._feed is None                 # a refused feed is not attached
    DeviceFeed(train, _data())
    # a captured step
    captured = _eval_step()
    captured.graph = object()
    with pytest.raises(ValueError, match="already been captured"):
        DeviceFeed(captured, _data())
    assert EvalStep._feed is None                                     # no feed: the class default, every path as before


def test_fields_that_share_a_static_buffer_are_one_field():
    """NACA's func_in IS its mesh_in (train_naca.py:62-65): one copy serves both, as in set_batch."""
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep

    class _Down:
        _batched = True

    model = _cpu_model()
    object.__setattr__(model, "down", _Down())                        # (only the mesh rule of the step looks at it)
    clouds = torch.zeros(8, 36, 2)
    step = EvalStep(model, (clouds, clouds, clouds, torch.zeros(8, 36, 1)), 1, 2)
    data = torch.rand(37, 36, 2)
    feed = DeviceFeed(step, {"mesh_in": data, "func_in": data, "mesh_out": data, "target": torch.rand(37, 36, 1)})
    assert feed.names == ["func_in", "target"] and len(feed.src) == len(feed.dst) == 2


def test_fields_that_share_a_static_buffer_must_bring_the_same_data():
    from position_induced_transformer_amd.engine import DeviceFeed, EvalStep

    class _Down:
        _batched = True

    model = _cpu_model()
    object.__setattr__(model, "down", _Down())
    clouds = torch.zeros(8, 36, 2)
    step = EvalStep(model, (clouds, clouds, clouds, torch.zeros(8, 36, 1)), 1, 2)
    with pytest.raises(ValueError, match="share one static buffer"):
        DeviceFeed(step, {"mesh_in": torch.rand(37, 36, 2), "func_in": torch.rand(37, 36, 2), "target": torch.rand(37, 36, 1)})
    assert step._feed is None


def test_a_step_with_a_feed_refuses_set_batch():
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    step = _eval_step()
    x = torch.ones(8, 36, 1)
    step.set_batch(x, x)                                              # no feed: as ever
    DeviceFeed(step, _data())
    with pytest.raises(RuntimeError, match="two sources"):
        step.set_batch(2 * x, 2 * x)
    assert torch.equal(step.func_in, x)                               # refused before anything was copied
    mesh, x0, _, y0 = _cpu_batch()
    train = TrainStep(_cpu_model(), (mesh, x0, mesh, y0), 1, 2)
    DeviceFeed(train, _data())
    with pytest.raises(RuntimeError, match="two sources"):
        train.set_batch(x, x)
