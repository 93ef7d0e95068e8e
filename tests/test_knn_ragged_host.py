"""No GPU: pit_knn_box on ragged batches (pit_knn_box_ragged; ops.knn_box / knn_box_restated / metric.knn_lists_box with
len_out / len_in) - the entry in header and binding, its refusals in pit_knn_box's order, the refusals of the Python side on CPU
tensors, and the numpy restatement with lengths against a per-sample stable sort of brute-force fp32 distances, exact."""
import ctypes
import re

import numpy as np
import pytest
import torch

from test_knn_host import BOX, HEADER, MAX_K, NULL, SIZE, UNSUPPORTED

NAN = float("nan")


def test_header_and_binding_carry_the_ragged_entry():
    from position_induced_transformer_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_KNN_RAGGED 1$", text, flags=re.M)
    assert _lib.DEFINES["PIT_HAS_KNN_RAGGED"] == 1 and _lib.ABI_VERSION == 31
    name = "pit_knn_box_ragged"
    assert name in _lib.ADDED_LATER and hasattr(_lib.lib(), name)
    # pit_knn_box's parameters with len_out / len_in between k and idx
    box, rag = _lib.PROTOTYPES["pit_knn_box"].argnames, _lib.PROTOTYPES[name].argnames
    at = box.index("idx")
    assert rag == box[:at] + ["len_out", "len_in"] + box[at:]


RAGGED_TABLE = [
    (dict(mesh_out=None), NULL), (dict(idx=None), NULL), (dict(next=None, batch=0), NULL),
    (dict(batch=0), SIZE), (dict(n_in=0), SIZE), (dict(space_dim=9), SIZE), (dict(out_stride=899), SIZE),
    (dict(k=0), SIZE), (dict(k=5001), SIZE),                              # k is checked against the PADDED width
    (dict(k=MAX_K + 1), UNSUPPORTED),
    (dict(k=5001, n_in=5000), SIZE),
]


@pytest.mark.parametrize("lens", ["both", "none"])
@pytest.mark.parametrize("change,code", RAGGED_TABLE, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in RAGGED_TABLE])
def test_entry_refuses_as_pit_knn_box_does(change, code, lens):
    from position_induced_transformer_amd import _lib
    a = dict(BOX, **change)
    p = BOX["idx"] if lens == "both" else None                           # (NULL lengths are the full width, not an error)
    got = _lib.lib().pit_knn_box_ragged(a["mesh_out"], a["mesh_in"], a["batch"], a["n_out"], a["n_in"], a["space_dim"], a["out_stride"],
                                        a["in_stride"], a["periods"], a["k"], p, p, a["idx"], a["dist"], a["next"], a["stream"])
    assert got == code
    assert got == _lib.lib().pit_knn_box(*(a[n] for n in _lib.PROTOTYPES["pit_knn_box"].argnames))


def test_python_refusals_come_before_the_device_check():
    from position_induced_transformer_amd import metric, ops
    clouds, shared = torch.rand(3, 20, 2), torch.rand(7, 2)
    for fn in (lambda **kw: ops.knn_box(kw.pop("mo"), kw.pop("mi"), 4, **kw), lambda **kw: ops.knn_box_restated(kw.pop("mo"), kw.pop("mi"), 4, **kw),
               lambda **kw: metric.knn_lists_box(kw.pop("mo"), kw.pop("mi"), 4, **kw)):
        with pytest.raises(ValueError, match="shared by the batch"):
            fn(mo=shared, mi=clouds, len_out=[7, 7, 7])
        with pytest.raises(ValueError, match="shared by the batch"):
            fn(mo=clouds, mi=shared, len_in=[7, 7, 7])
        with pytest.raises(ValueError, match="shared by the batch"):
            fn(mo=shared, mi=shared, len_in=[7])
        with pytest.raises(ValueError, match="one entry per sample"):
            fn(mo=clouds, mi=clouds, len_in=[7, 7])
        with pytest.raises(TypeError, match="int32 or int64"):
            fn(mo=clouds, mi=clouds, len_in=torch.tensor([7.0, 7.0, 7.0]))
        with pytest.raises(ValueError, match=r"k must be an integer in \[1, 20\]"):          # the padded width bounds k
            ops.knn_box_restated(clouds, clouds, 21, len_in=[20, 20, 20])
    with pytest.raises(RuntimeError, match="HIP device only"):           # every check passed: the device check is the next one
        ops.knn_box(clouds, clouds, 4, len_in=[20, 3, 1])


def _brute(x, y, periods):
    """fp32 distances of every row to every key, the header's operation order, one pair at a time."""
    d = np.empty((len(x), len(y)), np.float32)
    for i in range(len(x)):
        for j in range(len(y)):
            acc = None
            for a in range(x.shape[1]):
                t = np.abs(np.float32(x[i, a]) - np.float32(y[j, a]))
                if periods is not None and periods[a] is not None:
                    t = np.minimum(t, np.float32(periods[a]) - t)
                q = np.float32(t * t)
                acc = q if acc is None else np.float32(acc + q)
            d[i, j] = acc
    return d


K = 6
# (space_dim, periods, shared side, len_in of the three samples); the width is 11, k = 6: len_in covers 1, k - 1, k, k + 1, width
RESTATED = [
    (1, None, None, (1, K - 1, K)),
    (3, None, None, (K + 1, 11, 2)),
    (5, None, None, (K, 1, 11)),
    (3, (0.75, None, None), None, (11, K - 1, K + 1)),
    (1, (0.5,), None, (K, K + 1, 1)),
    (3, None, "out", (K - 1, 11, 1)),
    (5, (None, 0.75, None, None, 0.3), "out", (K + 1, K, 3)),
    (3, None, "in", None),
    (1, (0.5,), "in", None),
]


@pytest.mark.parametrize("case", RESTATED, ids=[f"s{c[0]}-{'box' if c[1] is None else 'wrap'}-shared_{c[2]}-{c[3]}" for c in RESTATED])
def test_restatement_with_lengths_is_the_per_sample_stable_sort(case):
    from position_induced_transformer_amd import ops
    sdim, periods, shared, len_in = case
    b, n_out, width = 3, 9, 11
    g = torch.Generator().manual_seed(7 + sdim)
    mo = torch.rand(n_out, sdim, generator=g) if shared == "out" else torch.rand(b, n_out, sdim, generator=g)
    mi = torch.rand(width, sdim, generator=g) if shared == "in" else torch.rand(b, width, sdim, generator=g)
    if mi.dim() == 3:
        mi[:, 3] = mi[:, 0]                                               # a duplicate key: a tie the index decides
    len_out = None if shared == "out" else (9, 1, 4)
    if len_in is not None:
        for s in range(b):
            mi[s, len_in[s]:] = NAN                                       # NaN in all padding
    if len_out is not None:
        for s in range(b):
            mo[s, len_out[s]:] = NAN
    got = ops.knn_box_restated(mo, mi, K, periods, len_out=len_out, len_in=len_in)
    assert got.idx.shape == (b, n_out, K) and got.dist.shape == (b, n_out, K) and got.next.shape == (b, n_out)
    assert got.idx.dtype == torch.int32 and got.dist.dtype == torch.float32
    for s in range(b):
        lo, li = (n_out if len_out is None else len_out[s]), (width if len_in is None else len_in[s])
        x = (mo if mo.dim() == 2 else mo[s]).numpy()[:lo]
        y = (mi if mi.dim() == 2 else mi[s]).numpy()[:li]
        d = _brute(x, y, periods)
        order = np.argsort(d, axis=-1, kind="stable")
        kk = min(K, li)
        assert np.array_equal(got.idx[s, :lo, :kk].numpy(), order[:, :kk].astype(np.int32))
        assert np.array_equal(got.dist[s, :lo, :kk].numpy().view(np.int32), np.take_along_axis(d, order, -1)[:, :kk].view(np.int32))
        nxt = np.take_along_axis(d, order, -1)[:, K] if K < li else np.full(lo, np.inf, np.float32)
        assert np.array_equal(got.next[s, :lo].numpy(), nxt)
        # what the search does not reach: key -1, distance 0; padded rows whole, with next = +inf
        assert (got.idx[s, :lo, kk:] == -1).all() and not got.dist[s, :lo, kk:].any()
        assert (got.idx[s, lo:] == -1).all() and not got.dist[s, lo:].any() and torch.isinf(got.next[s, lo:]).all()
    # the trimmed sample alone gives the same pairs (the statement the GPU test makes of the kernel)
    if len_in is not None and mo.dim() == 3:
        s = 1
        alone = ops.knn_box_restated(mo[s, :len_out[s]], mi[s, :len_in[s]], min(K, len_in[s]), periods)
        assert torch.equal(alone.idx, got.idx[s, :len_out[s], :min(K, len_in[s])])
        assert torch.equal(alone.next, got.next[s, :len_out[s]])


def test_lengths_are_clamped_into_the_width():
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(3)
    mo, mi = torch.rand(2, 5, 2, generator=g), torch.rand(2, 8, 2, generator=g)
    a = ops.knn_box_restated(mo, mi, 3, len_out=[0, 99], len_in=[-4, 99])
    b = ops.knn_box_restated(mo, mi, 3, len_out=[1, 5], len_in=[1, 8])
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    full = ops.knn_box_restated(mo, mi, 3)
    assert torch.equal(a.idx[1], full.idx[1]) and torch.equal(a.next[1], full.next[1])
