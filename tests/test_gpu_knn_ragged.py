"""GPU: pit_knn_box on ragged batches (ops.knn_box with len_out / len_in) against ops.knn_box on each TRIMMED sample: keys,
distances and `next` bit for bit, -1 / 0 in the slots a short sample does not fill, -1 / 0 / +inf in padded rows, NaN in all
padding, both forms of the kernel (chosen from the padded width), and one captured launch that follows lengths overwritten in
place.  No tolerance anywhere: the selection is exact."""
import pytest
import torch

from test_knn_host import REG_MAX

pytestmark = pytest.mark.gpu

NAN = float("nan")
B, N_OUT = 4, 37
PER = (None, 0.75, None)


def _lengths(n_in, k, seed):
    """len_in: the full width, 1, one key fewer than k (k > 1) and an odd count in between; len_out: 37, 1, 20, 36."""
    return [N_OUT, 1, 20, N_OUT - 1], [n_in, 1, max(1, k - 1), 517 + seed]


def _clouds(seed, n_in, layout, len_out, len_in):
    """Per-sample clouds with NaN in every padded point; layout: which side is the mesh shared by the batch."""
    g = torch.Generator().manual_seed(seed)
    mo = torch.rand(N_OUT, 3, generator=g) * 2.0 - 0.5 if layout == "shared_out" else torch.rand(B, N_OUT, 3, generator=g) * 2.0 - 0.5
    mi = torch.rand(n_in, 3, generator=g) * 2.0 - 0.5 if layout == "shared_in" else torch.rand(B, n_in, 3, generator=g) * 2.0 - 0.5
    if mi.dim() == 3:
        mi[:, 5] = mi[:, 2]                                               # a duplicate key: the index decides
    for s in range(B):
        if len_out is not None:
            mo[s, len_out[s]:] = NAN
        if len_in is not None:
            mi[s, len_in[s]:] = NAN
    return mo.cuda(), mi.cuda()


def _check_against_trimmed(got, mo, mi, k, len_out, len_in, n_in, tag):
    from position_induced_transformer_amd import ops
    assert got.idx.shape == (B, N_OUT, k) and got.dist.shape == (B, N_OUT, k) and got.next.shape == (B, N_OUT)
    assert got.idx.dtype == torch.int32
    for s in range(B):
        lo, li = (N_OUT if len_out is None else len_out[s]), (n_in if len_in is None else len_in[s])
        kk = min(k, li)
        x = (mo if mo.dim() == 2 else mo[s])[:lo]
        y = (mi if mi.dim() == 2 else mi[s])[:li]
        ref = ops.knn_box(x, y, kk, PER)
        assert torch.equal(got.idx[s, :lo, :kk], ref.idx), (tag, s)
        assert torch.equal(got.dist[s, :lo, :kk].view(torch.int32), ref.dist.view(torch.int32)), (tag, s)
        if k < li:                                                        # the trimmed run with k' = k has the same pair k + 1
            assert torch.equal(got.next[s, :lo].view(torch.int32), ref.next.view(torch.int32)), (tag, s)
        else:
            assert bool(torch.isinf(got.next[s, :lo]).all()) and bool((got.next[s, :lo] > 0).all()), (tag, s)
        assert bool((got.idx[s, :lo, kk:] == -1).all()) and not bool(got.dist[s, :lo, kk:].any()), (tag, s)
        assert bool((got.idx[s, lo:] == -1).all()) and not bool(got.dist[s, lo:].any()), (tag, s)
        assert bool(torch.isinf(got.next[s, lo:]).all()), (tag, s)
        assert bool((got.idx[s, :lo, :kk] >= 0).all()) and bool((got.idx[s, :lo, :kk] < li).all()), (tag, s)
    assert bool(torch.isfinite(got.dist).all())                          # no NaN of the padding reached a distance


@pytest.mark.parametrize("layout", ["both", "len_in_only", "shared_out", "shared_in"])
@pytest.mark.parametrize("k", [1, 33, 300])
@pytest.mark.parametrize("n_in", [REG_MAX, 1100])
def test_ragged_box_is_the_trimmed_samples_bit_for_bit(n_in, k, layout):
    from position_induced_transformer_amd import ops
    len_out, len_in = _lengths(n_in, k, k % 7)
    if layout in ("len_in_only", "shared_out"):
        len_out = None                                                    # NULL: the full width (a shared side takes none)
    if layout == "shared_in":
        len_in = None
    mo, mi = _clouds(100 + k, n_in, layout, len_out, len_in)
    got = ops.knn_box(mo, mi, k, PER, len_out=len_out, len_in=len_in)
    assert ops.knn_last_form() == (1 if n_in <= REG_MAX else 2)          # the form comes from the PADDED width
    _check_against_trimmed(got, mo, mi, k, len_out, len_in, n_in, (n_in, k, layout))


def test_full_lengths_are_the_dense_entry():
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(5)
    mo, mi = torch.rand(B, N_OUT, 2, generator=g).cuda(), torch.rand(B, 700, 2, generator=g).cuda()
    a = ops.knn_box(mo, mi, 48, (1.0, None))
    b = ops.knn_box(mo, mi, 48, (1.0, None), len_out=[N_OUT] * B, len_in=[700] * B)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("n_in", [REG_MAX, 1100])
def test_one_captured_launch_follows_lengths_overwritten_in_place(n_in):
    from position_induced_transformer_amd import ops
    k = 33
    sets = [_lengths(n_in, k, 0), ([3, N_OUT, 1, 9], [40, n_in, 700, 1]), ([N_OUT] * B, [n_in] * B)]
    g = torch.Generator().manual_seed(9)
    mo, mi = (torch.rand(B, N_OUT, 3, generator=g) * 2.0 - 0.5).cuda(), (torch.rand(B, n_in, 3, generator=g) * 2.0 - 0.5).cuda()
    lo = torch.tensor(sets[0][0], dtype=torch.int32, device="cuda")
    li = torch.tensor(sets[0][1], dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.knn_box(mo, mi, k, PER, len_out=lo, len_in=li)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.knn_box(mo, mi, k, PER, len_out=lo, len_in=li)
    for t in (1, 2, 0):
        lo.copy_(torch.tensor(sets[t][0], dtype=torch.int32)); li.copy_(torch.tensor(sets[t][1], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        _check_against_trimmed(res, mo, mi, k, sets[t][0], sets[t][1], n_in, (n_in, "replay", t))
