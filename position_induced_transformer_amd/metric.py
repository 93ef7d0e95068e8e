"""Position attention under a metric of the caller's own: the layers take squared distances, not a hard-wired metric.

The reference's extension point for another metric is overriding ``posatt.dist2att`` (pit.py:42-43,68-69); in this package such
a subclass runs on the composed torch path.  The layers here keep the fused HIP kernels instead: ``sqdist(mesh_out, mesh_in)``
is ordinary, differentiable torch code of the user's that returns the squared distances - (N, J), shared by the batch, or
(b, N, J) - and pit.py:48-57 is applied to that matrix by csrc/pit_distmat.hip (``ops.posatt_dist_apply``).  The layer returns
d loss / d m, so autograd differentiates through the metric, tie rules included: a mesh may require grad under ANY metric.

    # channel flow: periodic in x (period 2 pi), walls in y; a learnable latent mesh
    sq = sqdist_periodic_box((2 * math.pi, None))
    ltt = torch.rand(256, 2) * torch.tensor([2 * math.pi, 1.0])
    model = pit_metric(2, 1, 1, 64, 2, 2, ltt, 0.05, 0.05, sqdist=sq, learn_latent=True).cuda()
    out = model(mesh_in, func_in, mesh_out)            # (J, 2) / (b, J, 1) / (N, 2) -> (b, N, 1)
    out.square().sum().backward()                      # model.mesh_ltt.grad: through min(|dx|, l - |dx|) by autograd

Precomputed matrices (geodesic distances on a surface or a graph) go to ``forward_dist(m_dist, inputs)``.  The entries of a
matrix must be finite and >= 0; that is not checked (a check would synchronise).  fp32 math mode only; ragged batches on
candidate lists only (below).

Where the (N, J) matrix cannot be formed - a decoder of 11 271 x 728 points per sample, geodesics on 50 000 vertices - the layers
run on CANDIDATE LISTS instead: ``forward_list(idx, sqd, inputs)`` takes, per row, K slots (key, squared distance), (N, K) shared
by the batch or (b, N, K); a slot whose key is outside [0, J) is padding.  Memory is O(N K), J is unlimited, the kept set is the
dense layer's whenever the lists hold every key the dense layer keeps (``list_capacity(q, J)`` = k + 2 slots at least, more where
ties are expected), and the layer returns d loss / d sqd in the shape of ``sqd``.  ``knn_lists(sqdist, mesh_out, mesh_in, k)``
builds such lists from meshes under any metric with chunk x J peak memory and recomputes the listed distances differentiably,
so a mesh may require grad; ``pit_metric(..., neighbors="auto")`` runs its down and up layers that way.

    lists = knn_lists(sq, mesh_out, mesh_in, k=None, locality=0.02)     # NeighborLists(idx, sqd, cut_rows)
    out = layer.forward_list(lists.idx, lists.sqd, inputs)

``builder="hip"`` (layers and ``pit_metric``) builds the lists with the project's own kernels instead of dense blocks and
``torch.topk``: for ``sqdist_euclid`` and ``sqdist_periodic_box`` with float periods from the coordinates in one launch
(``knn_lists_box``, no N x J block at all), for any other metric by ``knn_lists(..., select="hip")``; among equal distances the
lowest key index is listed.  The default, "torch", is unchanged.

RAGGED BATCHES - per-sample clouds of different point counts, padded to one width - run on the candidate lists:
``forward_list(idx, sqd, inputs, lengths=)`` (or ``len_out=`` / ``len_in=``) on per-sample (b, N, K) lists,
``knn_lists_box(..., len_out=, len_in=)``, the layers' ``forward(..., lengths=)`` / ``forward(..., len_out=, len_in=)`` with
``neighbors`` set, ``builder="hip"`` and a box metric, and ``pit_metric.forward(mesh_in, func_in, mesh_out, len_in=, len_out=)``.
The lengths are int32 device tensors (``ops.as_lengths``) the kernels read: no synchronisation, one captured graph for every mix
of sizes.  Sample s comes out as the list layer computes that cloud alone; padded rows give zeros, padded points take no part and
receive zero gradients, and the padding may hold anything, NaN included.  Dense matrices (``forward_dist``), ``builder="torch"``,
metrics that are no box metric, per-sample latent meshes in ``pit_metric`` and the bf16 math mode do not take lengths.

GEODESIC LISTS - the metric is a path length on a graph (a surface's edges, or ``knn_graph`` of the cloud) - are built on the
device by ``knn_lists_geodesic(adj, w, k, ...)``: one launch of a truncated shortest-path search per row (ops.geo_knn), per-sample
graphs and lengths included, so the search stays inside a captured step.  ``pit_cloud_geodesic`` runs all three attention stages
on such lists.  The lists are constants: path lengths carry no gradient to the mesh or the edge weights.

Not part of ``pit.py``, whose star-exports are the reference's.
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple

import torch
import torch.nn as nn

from . import ops
from . import pit as _pit

__all__ = ["sqdist_euclid", "sqdist_periodic_box", "posatt_metric", "posatt_cross_metric", "pit_metric", "list_capacity",
           "NeighborLists", "knn_lists", "knn_lists_box", "knn_graph", "GeodesicLists", "knn_lists_geodesic", "pit_cloud_geodesic"]


def sqdist_euclid(mesh_out: torch.Tensor, mesh_in: torch.Tensor) -> torch.Tensor:
    """sum((mesh_out[:, None] - mesh_in[None]) ** 2, -1), the op sequence of pit.py:47 / :134; batched or batch-free meshes."""
    diff = mesh_out.unsqueeze(-2) - mesh_in.unsqueeze(-3)
    return torch.sum(diff ** 2, dim=-1)


sqdist_euclid.box_periods = None       # a box metric without a wrapped axis: builder="hip" builds its lists from coordinates


def sqdist_periodic_box(periods):
    """Squared distance on a box that is periodic in some axes: ``periods[k]`` is the period of coordinate k (a float or a
    0-d tensor) or None for an axis that does not wrap; any number of coordinates.  The wrapped axes follow the op sequence of
    pit.py:248-253 - d = |x - y|, d = minimum(d, l - d), sum of squares - so with every axis wrapped by the reference's own
    period the result is the reference's bit for bit."""
    periods = tuple(periods)

    def sqdist(mesh_out: torch.Tensor, mesh_in: torch.Tensor) -> torch.Tensor:
        if mesh_out.shape[-1] != len(periods) or mesh_in.shape[-1] != len(periods):
            raise ValueError(f"sqdist_periodic_box of {len(periods)} axes got meshes with {mesh_out.shape[-1]} / {mesh_in.shape[-1]} coordinates")
        d = abs(mesh_out.unsqueeze(-2) - mesh_in.unsqueeze(-3))
        if all(p is not None for p in periods) and all(p is periods[0] or p == periods[0] for p in periods):
            l = periods[0]                                  # one period for every axis: pit.py:251-253 literally
            d = torch.minimum(d, l - d)
        elif any(p is not None for p in periods):
            cols = []
            for k, p in enumerate(periods):
                dk = d[..., k]
                cols.append(dk if p is None else torch.minimum(dk, p - dk))
            d = torch.stack(cols, dim=-1)
        return torch.sum(d ** 2, dim=-1)
    sqdist.box_periods = periods       # (what builder="hip" hands to knn_lists_box when every period is a float or None)
    return sqdist


def list_capacity(locality: float, n_in: int) -> int:
    """Least list width ``forward_list`` accepts for a layer of ``locality`` over ``n_in`` keys: k + 2 with (k, w) =
    ops.quantile_rank(locality, n_in); 1 for locality 1.0 (no selection)."""
    return ops.list_capacity(locality, n_in)


def default_neighbors(locality: float, n_in: int) -> int:
    """List width ``knn_lists`` takes when none is given: list_capacity plus room for ties, in multiples of 16 (the rule of
    ops.ragged_list_capacity), at most ``n_in``."""
    want = list_capacity(locality, n_in)
    return min(int(n_in), ((want + max(16, want // 4) + 15) // 16) * 16)


NeighborLists = namedtuple("NeighborLists", ["idx", "sqd", "cut_rows"])


def _listed_sqdist(sqdist, mesh_out, mesh_in, idx, len_out=None, len_in=None):
    """``sqdist`` of the listed pairs only, the rows as its batch axis - sqdist((R, 1, s), (R, k, s)) -> (R, 1, k) - in the shape
    of ``idx``: O(N k) and differentiable.  With lengths (a ragged batch; ``idx`` holds -1 at padding) the metric sees real
    points only: a padding key is replaced by key 0 of its sample and a padded row by row 0 before the gather, through
    torch.where - so whatever the padded points hold (NaN included) neither reaches ``sqdist`` nor, as 0 * NaN, a gradient; the
    layer's d(sqd) is 0 at those pairs, so the stand-ins receive nothing either."""
    n_out, k, s = int(mesh_out.shape[-2]), int(idx.shape[-1]), mesh_out.shape[-1]
    if len_out is not None or len_in is not None:
        b, dev = idx.shape[0], idx.device
        ok = idx >= 0
        if len_in is not None:
            ok = ok & (idx < len_in.view(b, 1, 1))
        if len_out is not None:
            row_ok = torch.arange(n_out, device=dev).view(1, n_out) < len_out.view(b, 1)
            ok = ok & row_ok.unsqueeze(-1)
            mesh_out = torch.where(row_ok.unsqueeze(-1), mesh_out, mesh_out[:, :1])
        idx = torch.where(ok, idx, torch.zeros_like(idx))
        if len_in is not None:                               # (rows beyond the length are never gathered; keep NaN out of the backward's scatter)
            key_ok = torch.arange(mesh_in.shape[-2], device=dev).view(1, -1) < len_in.view(b, 1)
            mesh_in = torch.where(key_ok.unsqueeze(-1), mesh_in, mesh_in[:, :1])
    if mesh_out.dim() == 3 or mesh_in.dim() == 3:
        b = idx.shape[0]
        rows = (mesh_out if mesh_out.dim() == 3 else mesh_out.unsqueeze(0).expand(b, -1, -1)).reshape(b * n_out, 1, s)
        if mesh_in.dim() == 3:
            keys = mesh_in[torch.arange(b, device=idx.device).view(b, 1, 1), idx]
        else:
            keys = mesh_in[idx]
        keys = keys.reshape(b * n_out, k, s)
    else:
        rows, keys = mesh_out.unsqueeze(1), mesh_in[idx]
    return sqdist(rows, keys).reshape(idx.shape)


def _check_neighbors(k, locality: float, n_in: int) -> int:
    if k is None:
        k = default_neighbors(locality, n_in)
    k = int(k)
    need = list_capacity(locality, n_in)
    if not (need <= k <= n_in):
        raise ValueError(f"k = {k}: a layer of locality {locality} over {n_in} keys needs between {need} and {n_in} neighbours")
    return k


def _cut_rows(dist, nxt, k: int, n_in: int, locality: float):
    """knn_lists's count of rows whose list may be cut inside a tie shell, from a kernel's own (dist, next); no synchronisation."""
    if k >= n_in:
        return torch.zeros((), dtype=torch.int64, device=dist.device)
    if float(locality) >= 1.0:
        return torch.full((), nxt.numel(), dtype=torch.int64, device=dist.device)
    return (nxt <= dist[..., ops.quantile_rank(float(locality), n_in)[0] + 1]).sum()


def _sample_lengths(mesh_out, mesh_in, len_out, len_in):
    """The lengths of a ragged batch as (len_out, len_in) device tensors (None where not given); a length for a side whose mesh is
    shared by the batch is a ValueError (the rule of ops.check_mixed), raised before the device check."""
    if len_out is None and len_in is None:
        return None, None
    ops.check_knn_lengths(mesh_out, mesh_in, len_out, len_in)
    cloud = mesh_out if mesh_out.dim() == 3 else mesh_in
    return tuple(None if v is None else ops.as_lengths(v, cloud.device, cloud.shape[0]) for v in (len_out, len_in))


def _cut_rows_ragged(dist, nxt, k: int, n_out: int, n_in: int, locality: float, len_out, len_in):
    """``_cut_rows`` for a ragged batch: real rows only, each against the rank of ITS sample (ops.quantile_rank's fp32 arithmetic
    as torch ops on the device lengths - no synchronisation); a sample with no more than k keys lists them all: no cut rows."""
    b, dev = dist.shape[0], dist.device
    li = torch.full((b,), n_in, device=dev, dtype=torch.int64) if len_in is None else len_in.long().clamp(1, n_in)
    lo = torch.full((b,), n_out, device=dev, dtype=torch.int64) if len_out is None else len_out.long().clamp(1, n_out)
    real = (torch.arange(n_out, device=dev).view(1, n_out) < lo.view(b, 1)) & (li > k).view(b, 1)
    if float(locality) >= 1.0:
        return real.sum()
    # fl32(q) * fl32(li - 1), floor: an fp32 tensor times a Python scalar multiplies in fp32 (no host-to-device copy: capturable)
    rank = torch.floor(torch.mul((li - 1).to(torch.float32), float(locality))).long()
    at = (rank + 1).clamp(max=k - 1).view(b, 1, 1).expand(b, n_out, 1)
    return ((nxt <= dist.gather(-1, at).squeeze(-1)) & real).sum()


def knn_lists_box(mesh_out, mesh_in, k=None, periods=None, locality: float = 1.0, len_out=None, len_in=None) -> NeighborLists:
    """``knn_lists`` for a box metric - Euclidean, or periodic in the axes whose ``periods[a]`` is a float (None: the axis does
    not wrap) - with the keys from ONE launch of ops.knn_box: no N x J block is formed, no library sort runs, and among equal
    distances the lowest key index is taken.  ``idx`` (int64) lists a row's keys ascending by (distance, index); ``sqd`` is
    recomputed for the listed pairs by sqdist_euclid / sqdist_periodic_box(periods) as knn_lists does, so a mesh may require grad;
    ``cut_rows`` follows knn_lists's rule on the kernel's own distances, without a synchronisation.  ``k`` None:
    default_neighbors; at most 2048 (ops.KNN_MAX_K).  Every refusal is a ValueError raised before a launch.
    ``len_out`` / ``len_in``: a ragged batch (ops.knn_box with lengths) - ``k`` and its default come from the PADDED width;
    sample s lists min(k, len_in[s]) of its own keys, every other slot holds key -1 (padding to the list layers) and a finite
    ``sqd`` the layers never use; ``cut_rows`` counts real rows only, each against its sample's own rank."""
    for name, t in (("mesh_out", mesh_out), ("mesh_in", mesh_in)):
        if not torch.is_tensor(t) or t.dim() not in (2, 3) or 0 in t.shape:
            raise ValueError(f"{name} must be a non-empty (n, space_dim) or (b, n, space_dim) tensor")
    n_in = int(mesh_in.shape[-2])
    k = _check_neighbors(k, locality, n_in)
    if k > ops.KNN_MAX_K:
        raise ValueError(f"k = {k}: at most {ops.KNN_MAX_K} neighbours are supported (the width the list layers accept)")
    per = ops.check_knn_box_shapes(mesh_out, mesh_in, k, periods)[5]
    len_out, len_in = _sample_lengths(mesh_out, mesh_in, len_out, len_in)
    with torch.no_grad():
        got = ops.knn_box(mesh_out, mesh_in, k, periods, len_out=len_out, len_in=len_in)
        if len_out is None and len_in is None:
            cut = _cut_rows(got.dist, got.next, k, n_in, locality)
        else:
            cut = _cut_rows_ragged(got.dist, got.next, k, int(mesh_out.shape[-2]), n_in, locality, len_out, len_in)
        idx = got.idx.long()
    sqdist = sqdist_euclid if per is None else sqdist_periodic_box(tuple(p if p > 0.0 else None for p in per))
    return NeighborLists(idx, _listed_sqdist(sqdist, mesh_out, mesh_in, idx, len_out, len_in), cut)


def knn_lists(sqdist, mesh_out, mesh_in, k=None, chunk: int = 4096, locality: float = 1.0, select: str = "torch") -> NeighborLists:
    """The ``k`` nearest keys of every row under ``sqdist``: ``idx`` (int64) and ``sqd`` of shape (N, k), or (b, N, k) when a
    mesh is batched.  The keys come from dense distances of ``chunk`` rows at a time under no_grad (peak memory chunk x J) and
    ``torch.topk``; ``sqd`` is then recomputed for the chosen pairs only, by calling ``sqdist`` with the rows as its batch axis -
    sqdist((R, 1, s), (R, k, s)) -> (R, 1, k) - so autograd holds O(N k) and a mesh may require grad.  ``k`` None: list_capacity
    of ``locality`` plus room for ties (default_neighbors).  ``cut_rows``: a 0-d tensor on the meshes' device, computed without
    a synchronisation: the number of rows whose list may hold other keys than the dense layer of ``locality`` keeps - rows
    whose (k+1)-th nearest value is <= their m_(rank+1), i.e. a tie shell at the threshold reaches beyond the list; without a
    mask (locality 1.0) every row, unless the lists hold all J keys.  ``select``: "torch" - torch.topk, whose choice among equal
    distances is unspecified - or "hip": ops.knn_rows on the same chunks (k <= 2048), the lowest key index among equals and the
    lists ascending by (distance, index)."""
    if select not in ("torch", "hip"):
        raise ValueError(f"select must be 'torch' or 'hip', got {select!r}")
    n_in = int(mesh_in.shape[-2])
    k = _check_neighbors(k, locality, n_in)
    if select == "hip" and k > ops.KNN_MAX_K:
        raise ValueError(f"k = {k}: select='hip' supports at most {ops.KNN_MAX_K} neighbours")
    n_out = int(mesh_out.shape[-2])
    rank = ops.quantile_rank(float(locality), n_in)[0]
    with torch.no_grad():
        mo, mi = mesh_out.detach(), mesh_in.detach()
        parts, cut = [], None
        for r0 in range(0, n_out, int(chunk)):
            m = sqdist(mo[..., r0:r0 + int(chunk), :], mi)
            if select == "hip":
                got = ops.knn_rows(m, k)
                parts.append(got.idx)
                hit = _cut_rows(got.dist, got.next, k, n_in, locality)
                cut = hit if cut is None else cut + hit
                continue
            vals, ind = torch.topk(m, min(k + 1, n_in), dim=-1, largest=False, sorted=True)
            parts.append(ind[..., :k])
            if k < n_in:
                hit = (vals[..., k] <= vals[..., rank + 1]) if float(locality) < 1.0 else torch.ones_like(vals[..., k], dtype=torch.bool)
                cut = hit.sum() if cut is None else cut + hit.sum()
        idx = torch.cat(parts, dim=-2).long()
        if cut is None:
            cut = torch.zeros((), dtype=torch.int64, device=idx.device)
    return NeighborLists(idx, _listed_sqdist(sqdist, mesh_out, mesh_in, idx), cut)


def knn_graph(mesh, g: int, periods=None, lengths=None):
    """The directed ``g``-nearest-neighbour graph of a cloud as padded adjacency for ``knn_lists_geodesic`` / ops.geo_knn:
    ``adj`` (.., n, g + 1) int32 and ``w`` (.., n, g + 1) fp32 from ONE ops.knn_box(mesh, mesh, g + 1, ...), ``w = sqrt(dist)``
    - edge lengths, not their squares.  The self slot (length 0) is kept: a self edge is harmless to the search.  The graph is
    NOT symmetrised: u may list v without v listing u.  ``lengths``: a ragged batch of (b, n, s) clouds - padded points get no
    edges (key -1) and no vertex lists one.  A constant: nothing differentiates through it.  No synchronisation, capturable."""
    if isinstance(g, bool) or not isinstance(g, int) or g < 1:
        raise ValueError(f"g must be a positive integer, got {g!r}")
    with torch.no_grad():
        got = ops.knn_box(mesh, mesh, g + 1, periods, len_out=lengths, len_in=lengths)
        return got.idx, torch.sqrt(got.dist)


GeodesicLists = namedtuple("GeodesicLists", ["idx", "sqd", "cut_rows", "truncated_rows", "short_rows"])


def _cut_rows_geo(got, k: int, n_vert: int, locality: float, sources, key_of, len_v):
    """``_cut_rows_ragged`` where the rows and keys of a sample are not prefixes but what the search saw: real rows are those
    whose source is a vertex of the sample, a sample's key count is counted from ``key_of`` below its length.  No
    synchronisation."""
    b, n_rows = got.next.shape
    dev = got.next.device
    vs = len_v.long().clamp(1, n_vert).view(b, 1)
    below = torch.arange(n_vert, device=dev).view(1, n_vert) < vs
    li = vs.view(b) if key_of is None else ((key_of.reshape(-1, n_vert) >= 0) & below).sum(-1).expand(b)
    src = torch.arange(n_vert, device=dev).view(1, n_vert) if sources is None else sources.reshape(-1, n_rows)
    real = ((src >= 0) & (src < vs)).expand(b, n_rows) & (li > k).view(b, 1)
    if float(locality) >= 1.0:
        return real.sum()
    rank = torch.floor(torch.mul((li - 1).clamp(min=0).to(torch.float32), float(locality))).long()
    at = (rank + 1).clamp(max=k - 1).view(b, 1, 1).expand(b, n_rows, 1)
    return ((got.next <= got.dist.gather(-1, at).squeeze(-1)) & real).sum()


def knn_lists_geodesic(adj, w, k=None, locality: float = 1.0, sources=None, key_of=None, n_keys=None, len_v=None,
                       reach=None) -> GeodesicLists:
    """Candidate lists under the PATH LENGTH of a graph, from ONE launch of ops.geo_knn (a truncated shortest-path search per
    row; its arguments are that op's): ``idx`` (int64) lists a row's nearest reachable keys ascending by (length, vertex index),
    -1 (padding to the list layers) in the slots it does not fill; ``sqd = dist * dist`` (fp32) is the squared path length the
    layers take.  The lists are CONSTANTS: path lengths carry no gradient to edge weights or mesh coordinates - weights that
    require grad under grad mode raise NotImplementedError.
      n_keys     the number of keys J the lists index: needed with ``key_of`` (which must map onto [0, J), no key twice), V
                 without it.  ``k`` None: default_neighbors(locality, J).
      cut_rows   knn_lists's count from the search's own (dist, next).  ``next`` is exact when every vertex is a key and a lower
                 bound otherwise, so with ``key_of`` the count is an upper bound.  Truncated rows are not in it.
      truncated_rows   0-d device tensor: rows that met the ``reach`` budget.  They list fewer keys than asked - exactly, but
                 a layer then sees a shorter neighbourhood: raise ``reach`` (at most 4096) until this is 0.
      short_rows 0-d device tensor: real, complete rows with fewer than ``k`` keys - fewer keys are reachable (another component
                 of the graph, a short sample).  A MASKED layer (locality < 1) needs k' + 2 valid slots per row, k' its rank
                 (ListPlan's precondition, the caller's to keep): with short_rows > 0 that holds only if the short rows still
                 reach that many keys; an unmasked layer attends over what is listed.
    Every refusal is a ValueError raised before a launch.  No synchronisation, capturable."""
    if torch.is_tensor(w) and w.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("edge weights that require grad: the geodesic lists are constants - path lengths carry no "
                                  "gradient (detach the weights)")
    if not torch.is_tensor(adj) or adj.dim() not in (2, 3) or 0 in adj.shape:
        raise ValueError("adj must be a non-empty (V, G) or (b, V, G) tensor")
    n_vert = int(adj.shape[-2])
    if key_of is None:
        if n_keys is not None and int(n_keys) != n_vert:
            raise ValueError(f"n_keys = {n_keys} without key_of: every one of the {n_vert} vertices is a key")
        n_keys = n_vert
    elif n_keys is None or isinstance(n_keys, bool) or int(n_keys) < 1 or int(n_keys) > n_vert:
        raise ValueError(f"key_of needs n_keys, the number of keys it maps onto, in [1, {n_vert}]; got {n_keys!r}")
    n_keys = int(n_keys)
    k = _check_neighbors(k, locality, n_keys)
    if k > ops.GEO_MAX_K:
        raise ValueError(f"k = {k}: at most {ops.GEO_MAX_K} neighbours are supported by the geodesic builder")
    batch = ops.check_geo_shapes(adj, w, k, sources, key_of, len_v, reach)[0]
    with torch.no_grad():
        if len_v is not None:
            len_v = ops.as_lengths(len_v, adj.device, batch)
        got = ops.geo_knn(adj, w, k, sources, key_of, len_v, reach)
        if len_v is None:
            cut = _cut_rows(got.dist, got.next, k, n_keys, locality)
        else:
            cut = _cut_rows_geo(got, k, n_vert, locality, sources, key_of, len_v)
        truncated = (got.status == 1).sum()
        short = ((got.status == 0) & (got.idx[..., k - 1] < 0) & _geo_real_rows(got, sources, len_v, n_vert)).sum()
        idx = got.idx.long()
        sqd = got.dist * got.dist
    return GeodesicLists(idx, sqd, cut, truncated, short)


def _geo_real_rows(got, sources, len_v, n_vert: int):
    """Mask of the rows whose source is a vertex of its sample, in the shape of ``got.next``."""
    src = torch.arange(n_vert, device=got.next.device) if sources is None else sources
    hi = n_vert if len_v is None else len_v.long().clamp(1, n_vert).view(-1, 1)
    return ((src >= 0) & (src < hi)).expand(got.next.shape)


class posatt_metric(nn.Module):
    """Self attention under ``sqdist``: ``forward(mesh, inputs)`` returns ``cat((inputs, conv), -1)`` as posatt.forward does
    (pit.py:37-44).  A plain module with an ``lmda`` parameter initialised as posatt's is (pit.py:35)."""

    _PLAN_CACHE = 8
    _self_attn = True

    def __init__(self, n_head, in_dim, locality, sqdist=sqdist_euclid, neighbors=None, builder: str = "torch"):
        super().__init__()
        if not (neighbors is None or neighbors == "auto" or (isinstance(neighbors, int) and neighbors > 0)):
            raise ValueError(f"neighbors must be None, 'auto' or a positive int, got {neighbors!r}")
        if builder not in ("torch", "hip"):
            raise ValueError(f"builder must be 'torch' or 'hip', got {builder!r}")
        self.builder = builder                # who builds the kNN lists: "torch" (dense chunks + topk) or "hip" (ops.knn_box / knn_rows)
        self.neighbors = neighbors            # None: dense distances; otherwise forward() builds kNN lists of that width
        self.last_lists = None                # the NeighborLists of the latest forward() on lists (cut_rows is read from here)
        self.locality = locality
        self.n_head = n_head
        self.in_dim = in_dim
        self.sqdist = sqdist
        self.lmda = nn.Parameter(torch.rand(n_head, 1, 1))
        self._plans = OrderedDict()          # LRU of plans of shared (N, J) matrices

    @staticmethod
    def _refuse_lengths(lengths):
        if lengths is not None:
            raise NotImplementedError("lengths (ragged batches) with a caller-supplied distance matrix are not implemented")

    def _cached_plan(self, key, build):
        """A plan of tensors the caller keeps and shares over the batch stays: least recently used first out (the plan holds
        its tensors, so their addresses cannot be handed to other tensors while the entry lives).  key None: not kept."""
        if key is None:
            return build()
        plan = self._plans.get(key)
        if plan is None:
            plan = build()
            while len(self._plans) >= self._PLAN_CACHE:
                self._plans.popitem(last=False)
            self._plans[key] = plan
        else:
            self._plans.move_to_end(key)
        if ops._capturing():
            ops._pin(plan)
        return plan

    def _plan(self, m_dist: torch.Tensor) -> ops.DistPlan:
        """A shared (N, J) matrix keeps its plan: keyed on address, shape, version and locality."""
        key = None if m_dist.dim() != 2 else (m_dist.data_ptr(), tuple(m_dist.shape), tuple(m_dist.stride()), m_dist._version,
                                              float(self.locality), m_dist.device.index)
        return self._cached_plan(key, lambda: ops.DistPlan(m_dist, self.locality))

    def forward_dist(self, m_dist, inputs, lengths=None):
        """The layer on a precomputed matrix of squared distances, (N, J) or (b, N, J)."""
        self._refuse_lengths(lengths)
        ops._check_dist_mode()
        ops.check_dist_shapes(m_dist, inputs, self._self_attn)
        plan = self._plan(m_dist)
        return ops.posatt_dist_apply(inputs, self.lmda, plan, self.n_head, concat=self._self_attn, m_dist=m_dist)

    def _list_plan(self, idx, sqd, n_in: int) -> ops.ListPlan:
        """Shared (N, K) lists keep their plan like a shared matrix does: keyed on both addresses, shapes, versions and locality."""
        key = None if idx.dim() != 2 else ("list", idx.data_ptr(), sqd.data_ptr(), tuple(idx.shape), tuple(idx.stride()),
                                           tuple(sqd.stride()), idx._version, sqd._version, int(n_in), float(self.locality), sqd.device.index)
        return self._cached_plan(key, lambda: ops.ListPlan(idx, sqd, n_in, self.locality))

    def forward_list(self, idx, sqd, inputs, lengths=None, len_out=None, len_in=None):
        """The layer on candidate lists: ``idx`` (int32 / int64) and ``sqd`` (fp32), (N, K) or (b, N, K); slot (i, t) says that
        key idx[i, t] lies at squared distance sqd[i, t] from row i; a key outside [0, J) marks padding.  K >= list_capacity(
        locality, J).  The self form (this class) needs N == J and prepends the inputs.
        ``len_out`` / ``len_in`` (``lengths``: both, the self form): a ragged batch on per-sample (b, N, K) lists - sample s has
        len_out[s] rows and len_in[s] keys and comes out as ``forward_list(idx[s, :len_out[s]], sqd[s, :len_out[s]],
        inputs[s:s+1, :len_in[s]])`` gives it; rows beyond are zero in every head column (the self form copies their inputs),
        keys >= len_in[s] are padding, and whatever the padding holds (NaN included) is never used.  K is checked against the
        padded J.  Such a plan follows its length tensors and is not kept in the cache."""
        if lengths is not None:
            if len_out is not None or len_in is not None:
                raise ValueError("give either lengths (both sides) or len_out / len_in")
            len_out = len_in = lengths
        ops._check_dist_mode()
        ops.check_list_shapes(idx, sqd, inputs, self._self_attn)
        if len_out is not None or len_in is not None:
            ops.check_list_lengths(idx, len_out, len_in)
            plan = ops.ListPlan(idx, sqd, inputs.shape[1], self.locality, len_out=len_out, len_in=len_in)
        else:
            plan = self._list_plan(idx, sqd, inputs.shape[1])
        return ops.posatt_list_apply(inputs, self.lmda, plan, self.n_head, concat=self._self_attn, sqd=sqd)

    def _build_lists(self, mesh_out, mesh_in, k):
        """builder "torch": knn_lists as ever.  "hip": a ``sqdist`` that says it is a box metric (``box_periods``: None, or per
        axis a float or None) gets its lists from coordinates (knn_lists_box); any other metric from ops.knn_rows on its chunks."""
        if self.builder == "torch":
            return knn_lists(self.sqdist, mesh_out, mesh_in, k, locality=self.locality)
        box, per = self._box_periods()
        if box:
            return knn_lists_box(mesh_out, mesh_in, k, periods=per, locality=self.locality)
        return knn_lists(self.sqdist, mesh_out, mesh_in, k, locality=self.locality, select="hip")

    RAGGED_SUPPORT = ("lengths (ragged batches) on the metric layers run on candidate lists built by the project's own kernels "
                      "for a box metric: neighbors set, builder='hip' and sqdist_euclid or sqdist_periodic_box with float periods "
                      "(or forward_list with lengths on lists of the caller's); ")

    def _box_periods(self):
        """(True, periods) when ``sqdist`` says it is a box metric whose periods the box kernel takes, else (False, None)."""
        if hasattr(self.sqdist, "box_periods"):
            per = self.sqdist.box_periods
            if per is None or all(p is None or (isinstance(p, (int, float)) and not isinstance(p, bool)) for p in per):
                return True, per
        return False, None

    def _on_meshes_ragged(self, mesh_out, mesh_in, inputs, len_out, len_in):
        """The layer on lists built for a ragged batch; every refusal before a launch."""
        if self.neighbors is None:
            raise NotImplementedError(self.RAGGED_SUPPORT + "dense distance matrices (neighbors=None) do not take lengths")
        if self.builder != "hip":
            raise NotImplementedError(self.RAGGED_SUPPORT + "builder='torch' does not take lengths")
        box, per = self._box_periods()
        if not box:
            raise NotImplementedError(self.RAGGED_SUPPORT + "this metric carries no box_periods with float periods")
        for name, t in (("mesh_out", mesh_out), ("mesh_in", mesh_in)):
            if not torch.is_tensor(t) or t.dim() not in (2, 3):
                raise ValueError(f"{name} must be a (n, space_dim) or (b, n, space_dim) tensor")
        len_out, len_in = _sample_lengths(mesh_out, mesh_in, len_out, len_in)
        lists = knn_lists_box(mesh_out, mesh_in, None if self.neighbors == "auto" else self.neighbors, periods=per,
                              locality=self.locality, len_out=len_out, len_in=len_in)
        self.last_lists = lists
        ops.check_list_shapes(lists.idx, lists.sqd, inputs, self._self_attn)
        plan = ops.ListPlan(lists.idx, lists.sqd, inputs.shape[1], self.locality, len_out=len_out, len_in=len_in)
        return ops.posatt_list_apply(inputs, self.lmda, plan, self.n_head, concat=self._self_attn, sqd=lists.sqd)

    def _on_meshes(self, mesh_out, mesh_in, inputs):
        # distances formed for this call - kNN lists (pit_metric(..., neighbors=...)) or the whole matrix: their plan is built
        # for this call too, like every per-sample mesh plan (the cache of forward_dist / forward_list is for what the caller keeps)
        if self.neighbors is not None:
            lists = self._build_lists(mesh_out, mesh_in, None if self.neighbors == "auto" else self.neighbors)
            self.last_lists = lists
            ops.check_list_shapes(lists.idx, lists.sqd, inputs, self._self_attn)
            plan = ops.ListPlan(lists.idx, lists.sqd, inputs.shape[1], self.locality)
            return ops.posatt_list_apply(inputs, self.lmda, plan, self.n_head, concat=self._self_attn, sqd=lists.sqd)
        m_dist = self.sqdist(mesh_out, mesh_in)
        ops.check_dist_shapes(m_dist, inputs, self._self_attn)
        plan = ops.DistPlan(m_dist, self.locality)
        return ops.posatt_dist_apply(inputs, self.lmda, plan, self.n_head, concat=self._self_attn, m_dist=m_dist)

    def forward(self, mesh, inputs, lengths=None):
        """``lengths``: a ragged batch of per-sample clouds (b, n, space_dim) - see ``_on_meshes_ragged`` for what takes them."""
        ops._check_dist_mode()
        if lengths is not None:
            return self._on_meshes_ragged(mesh, mesh, inputs, lengths, lengths)
        return self._on_meshes(mesh, mesh, inputs)

    def dist2att(self, m_dist, scale, locality):
        """Dense attention weights ((b,) H, N, J) of pit.py:48-52 on ``m_dist``: the fused kernel run on the identity as values,
        as posatt.dist2att builds them (``scale`` is the lmda parameter)."""
        ops._check_dist_mode()
        plan = ops.DistPlan(m_dist, float(locality))
        eye = torch.eye(plan.n_in, device=m_dist.device).unsqueeze(0).repeat(plan.mesh_batch, 1, 1)
        att = ops.posatt_dist_apply(eye, scale, plan, self.n_head, concat=False, m_dist=m_dist)
        att = att.reshape(plan.mesh_batch, plan.n_out, self.n_head, plan.n_in).permute(0, 2, 1, 3)
        return att if m_dist.dim() == 3 else att[0]


class posatt_cross_metric(posatt_metric):
    """Cross attention mesh_in -> mesh_out under ``sqdist`` (posatt_cross.forward, pit.py:63-71)."""

    _self_attn = False

    def forward(self, mesh_out, mesh_in, inputs, out_bf16: bool = False, len_out=None, len_in=None):
        """``len_out`` / ``len_in``: the point counts of the per-sample sides of a ragged batch; either mesh may be the 2-d one
        shared by the batch, which takes no length."""
        ops._check_dist_mode()
        if len_out is not None or len_in is not None:
            return self._on_meshes_ragged(mesh_out, mesh_in, inputs, len_out, len_in)
        return self._on_meshes(mesh_out, mesh_in, inputs)


class pit_metric(_pit.pit):
    """``pit.pit`` whose down / conv[i] / up are the metric layers above.  ``pit.encoder / processor / decoder`` call replaced
    modules as they are; none of the fused launches takes these layers.  ``forward(mesh_in, func_in, mesh_out)`` is the
    fixed-mesh task forward: the coordinates of ``mesh_in`` are prepended to ``func_in`` (train_darcy.py:51-55).
    ``learn_latent``: the latent mesh becomes a parameter.  ``neighbors``: an int, or "auto" for default_neighbors - down and up
    then build kNN lists under ``sqdist`` (knn_lists) and run on them (forward_list), O(N k) instead of O(N J); conv stays dense
    on the latent mesh.  None: dense distances everywhere.  ``builder``: "torch" (dense chunks and torch.topk) or "hip" - the lists come
    from the project's own kernels: from coordinates for sqdist_euclid / sqdist_periodic_box with float periods (no N x J block),
    from ops.knn_rows on the chunks for any other metric.

    Ragged batches: ``forward(mesh_in, func_in, mesh_out, len_in=, len_out=)`` with per-sample clouds (b, n, space_dim) against
    the latent mesh, which is shared by the batch and has no length - with ``neighbors`` set, ``builder="hip"`` and a box metric
    (posatt_metric.RAGGED_SUPPORT).  The processor is the dense one on the latent mesh, unchanged; ``learn_latent`` works."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc, sqdist=sqdist_euclid,
                 learn_latent: bool = False, neighbors=None, builder: str = "torch"):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc)
        self.down = posatt_cross_metric(self.n_head, self.in_dim, self.en_local, sqdist, neighbors, builder)
        self.conv = nn.ModuleList([posatt_metric(self.n_head, self.hid_dim, 1.0, sqdist) for _ in range(self.n_blocks)])
        self.up = posatt_cross_metric(self.n_head, self.hid_dim, self.de_local, sqdist, neighbors, builder)
        if learn_latent:
            self.mesh_ltt = nn.Parameter(self.mesh_ltt.detach().clone())

    # pit.encoder / decoder send a shared mesh against clouds with lengths through ops.check_mixed, whose refusals (space_dim > 3,
    # non-Euclidean metrics, mesh gradients) belong to the Euclidean ragged kernels: the metric layers take the lengths themselves
    def encoder(self, mesh_in, func_in, mesh_ltt, len_in=None, len_ltt=None):
        if len_in is None and len_ltt is None:
            return super().encoder(mesh_in, func_in, mesh_ltt)
        if len_ltt is not None:
            raise ValueError("a length for the latent mesh: pit_metric's latent mesh is shared by the batch and has no length")
        return self._mlp_gelu(self.en_layer, self.down(mesh_ltt, mesh_in, func_in, len_in=len_in))

    def decoder(self, mesh_ltt, func_ltt, mesh_out, len_ltt=None, len_out=None):
        if len_ltt is None and len_out is None:
            return super().decoder(mesh_ltt, func_ltt, mesh_out)
        if len_ltt is not None:
            raise ValueError("a length for the latent mesh: pit_metric's latent mesh is shared by the batch and has no length")
        return self.de(self.up(mesh_out, mesh_ltt, func_ltt, len_out=len_out))

    def forward(self, mesh_in, func_in, mesh_out, len_in=None, len_out=None):
        """``len_in`` / ``len_out``: the point counts of the clouds ``mesh_in`` / ``mesh_out`` (b, n, space_dim) of a ragged batch
        (None = full width; ``len_in`` alone serves both when ``mesh_out`` IS ``mesh_in``).  Padded rows of the result are
        finite (the decoder MLP's bias path) and meaningless: mask them, e.g. with ``RelLpNorm(...)(true, pred, lengths)``."""
        if len_out is None and len_in is not None and mesh_out is mesh_in:
            len_out = len_in
        mesh_ltt = self.mesh_ltt.to(func_in.device) if self.mesh_ltt.device != func_in.device else self.mesh_ltt
        coords = mesh_in if mesh_in.dim() == 3 else mesh_in.unsqueeze(0).expand(func_in.shape[0], -1, -1)
        func = torch.cat((coords, func_in), dim=-1)
        func = self.encoder(mesh_in, func, mesh_ltt, len_in=len_in)
        func = self.processor(func, mesh_ltt)
        return self.decoder(mesh_ltt, func, mesh_out, len_out=len_out)


class pit_cloud_geodesic(_pit.pit):
    """Per-sample clouds whose three attention stages all run on GEODESIC neighbourhoods: path lengths on a graph over the
    cloud's points (a surface's edges given by the caller, or the cloud's own ``graph_neighbors``-nearest-neighbour graph), so
    the two sides of a thin wall or the two arms of a C-shaped plate are far apart although they are close in space.  Glue over
    ``knn_lists_geodesic`` and the list layers; no kernels of its own.
      latent     ``n_latent`` points of every cloud by ops.farthest_point_sample (``start``): vertices of the graph
      down       sources = the latent points, keys = all vertices, locality ``en_loc``
      processor  every block is ``posatt_metric(..., 1.0).forward_list`` on ONE set of latent-to-latent lists of width
                 min(n_latent, proc_neighbors): attention over geodesic NEIGHBOURHOODS.  This is a different function from the
                 dense processor of ``pit`` / ``pit_metric``, which attends over every latent point.
      up         sources = all vertices, keys = the latent points, locality ``de_loc``
    ``func_in`` is fed to the encoder as it is (``in_dim`` channels, coordinates included if wanted).  ``reach``: the search
    budget of all three builds (None: ops.geo_default_reach of each width).  ``last_lists``: the three GeodesicLists (down,
    processor, up) of the latest forward - read ``truncated_rows`` / ``short_rows`` there.  Preconditions (ListPlan's, the
    caller's): the cloud holds at least ``n_latent`` distinct points, and every real row of a masked layer reaches its rank + 2
    keys.  fp32 math mode only; path lengths carry no mesh gradient."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, n_latent, en_loc, de_loc, graph_neighbors: int = 8,
                 proc_neighbors: int = 64, reach=None, start=0):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, None, en_loc, de_loc)
        for name, v in (("n_latent", n_latent), ("graph_neighbors", graph_neighbors), ("proc_neighbors", proc_neighbors)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if reach is not None and (isinstance(reach, bool) or not isinstance(reach, int) or not 1 <= reach <= ops.GEO_MAX_REACH):
            raise ValueError(f"reach must be None or an integer in [1, {ops.GEO_MAX_REACH}], got {reach!r}")
        self.n_latent, self.graph_neighbors, self.proc_neighbors = n_latent, graph_neighbors, proc_neighbors
        self.reach, self.start = reach, start
        self.last_lists = self.last_latent = None
        self.down = posatt_cross_metric(self.n_head, self.in_dim, self.en_local)
        self.en_layer = _pit.kaiming_mlp(self.n_head * self.in_dim, self.hid_dim, self.hid_dim)
        self.conv = nn.ModuleList([posatt_metric(self.n_head, self.hid_dim, 1.0) for _ in range(self.n_blocks)])
        self.up = posatt_cross_metric(self.n_head, self.hid_dim, self.de_local)

    def forward(self, mesh_in, func_in, mesh_out, len_in=None, adj=None, adj_w=None):
        """``mesh_in`` (b, n, space_dim): the clouds, padded; ``mesh_out`` must BE ``mesh_in`` (query points are graph vertices);
        ``len_in``: the point counts of a ragged batch (None = full width); ``adj`` / ``adj_w``: the caller's graph as padded
        adjacency ((n, G) or (b, n, G), ops.geo_knn's format; edge LENGTHS, not squares), None: the kNN graph of ``mesh_in``.
        Padded rows of the result are finite and meaningless: mask them, e.g. with ``RelLpNorm(...)(true, pred, lengths)``."""
        if not torch.is_tensor(mesh_in) or mesh_in.dim() != 3:
            raise ValueError("pit_cloud_geodesic needs per-sample (batch, n, space_dim) clouds")
        same = mesh_out is mesh_in or (torch.is_tensor(mesh_out) and mesh_out.shape == mesh_in.shape
                                       and mesh_out.stride() == mesh_in.stride() and mesh_out.device == mesh_in.device
                                       and mesh_out.data_ptr() == mesh_in.data_ptr())
        if not same:
            raise ValueError("pit_cloud_geodesic: mesh_out must be mesh_in - query points must be vertices of the graph")
        if (adj is None) != (adj_w is None):
            raise ValueError("give both adj and adj_w (the graph and its edge lengths) or neither")
        b, n, _ = mesh_in.shape
        if self.n_latent > n:
            raise ValueError(f"n_latent = {self.n_latent} beyond the {n} points of a cloud")
        if adj is None and self.graph_neighbors + 1 > n:
            raise ValueError(f"graph_neighbors = {self.graph_neighbors}: a cloud of {n} points has at most {n - 1} neighbours")
        ops._check_dist_mode()
        m, kp = self.n_latent, min(self.n_latent, self.proc_neighbors)
        len_v = None if len_in is None else ops.as_lengths(len_in, mesh_in.device, b)
        if adj is None:
            adj, adj_w = knn_graph(mesh_in, self.graph_neighbors, lengths=len_v)
        with torch.no_grad():
            latent = ops.farthest_point_sample(mesh_in, m, len_v, self.start)
            # key_of: a device scatter of arange over the picks (a pick of -1, beyond a short cloud's, lands in a spare column)
            picks = latent.idx.long()
            key_of = torch.full((b, n + 1), -1, device=mesh_in.device, dtype=torch.int32)
            key_of.scatter_(1, torch.where(picks >= 0, picks, torch.full_like(picks, n)),
                            torch.arange(m, device=mesh_in.device, dtype=torch.int32).expand(b, m))
            key_of = key_of[:, :n].contiguous()
        len_l = latent.lengths
        down = knn_lists_geodesic(adj, adj_w, None, self.en_local, sources=latent.idx, n_keys=n, len_v=len_v, reach=self.reach)
        proc = knn_lists_geodesic(adj, adj_w, kp, 1.0, sources=latent.idx, key_of=key_of, n_keys=m, len_v=len_v, reach=self.reach)
        up = knn_lists_geodesic(adj, adj_w, None, self.de_local, key_of=key_of, n_keys=m, len_v=len_v, reach=self.reach)
        self.last_lists, self.last_latent = (down, proc, up), latent
        if len_v is None:
            ltt = self._mlp_gelu(self.en_layer, self.down.forward_list(down.idx, down.sqd, func_in))
            for a, w in zip(self.conv, self.mlp):
                ltt = self._mlp_gelu(w, a.forward_list(proc.idx, proc.sqd, ltt))
            return self.de(self.up.forward_list(up.idx, up.sqd, ltt))
        ltt = self._mlp_gelu(self.en_layer, self.down.forward_list(down.idx, down.sqd, func_in, len_out=len_l, len_in=len_v))
        for a, w in zip(self.conv, self.mlp):
            ltt = self._mlp_gelu(w, a.forward_list(proc.idx, proc.sqd, ltt, lengths=len_l))
        return self.de(self.up.forward_list(up.idx, up.sqd, ltt, len_out=len_v, len_in=len_l))
