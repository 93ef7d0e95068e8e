#!/usr/bin/env python3
"""What building the metric layers' neighbour lists costs on the device, per builder, in ONE process.

    python tools/knn_time.py [--replays 200] [--large-replays 3] [--repeats 9] [--shapes 0,1,2,3]

Three builders of the same lists under the Euclidean metric in 2-d (uniform points in the unit square), each captured into a
hipGraph of its own:
  torch   metric.knn_lists(select="torch"): dense chunks of 4096 rows, torch.topk(k + 1), the listed distances recomputed
  rows    metric.knn_lists(select="hip"):   the same chunks, ops.knn_rows (pit_knn_rows) in place of topk
  box     metric.knn_lists_box:             ops.knn_box (pit_knn_box) on the coordinates, no N x J block
at (N 256, J 700) and (N 900, J 256), locality 0.05 - the down and up layers of the model of tests/test_gpu_distlist.py -,
(N 11271, J 728) at 0.02 and N = J = 50000 at 0.02, with k = metric.default_neighbors.  Every graph holds the whole build: the
selection, the int64 keys, cut_rows and the recomputed distances.

After a warm-up block the blocks of bare replays alternate between the three graphs, one synchronisation per block; every figure
is the median block over `--repeats`, divided by the replays.  `--replays` per block at the first three shapes; at N = J = 50000 a
build takes from milliseconds to seconds, so its blocks hold `--large-replays`.  Also reported, not timed: the share of rows on
which a builder lists the same key set as `torch`, and each builder's cut_rows.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
from timeit import default_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, J, locality, large)
SHAPES = ((256, 700, 0.05, False), (900, 256, 0.05, False), (11271, 728, 0.02, False), (50000, 50000, 0.02, True))


def _median_us(graphs, replays: int, repeats: int):
    """{name: (median microseconds per replay, the blocks)} of graphs replayed in alternating blocks; block 0 is the warm-up."""
    import torch
    times = {name: [] for name in graphs}
    for rep in range(repeats + 1):
        for name, replay in graphs.items():
            torch.cuda.synchronize()
            t0 = default_timer()
            for _ in range(replays):
                replay()
            torch.cuda.synchronize()
            if rep:
                times[name].append(default_timer() - t0)
    return {name: (1e6 * statistics.median(t) / replays, [round(1e6 * v / replays, 2) for v in t]) for name, t in times.items()}


def _capture(fn):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return graph, keep


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--large-replays", type=int, default=3, help="replays per block at N = J = 50000")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--shapes", default="0,1,2,3", help="comma-separated indices into the shape list")
    args = ap.parse_args()
    import torch
    from position_induced_transformer_amd import metric, ops
    if not torch.cuda.is_available():
        raise SystemExit("tools/knn_time.py measures on the HIP device; none found")
    out = {"replays": args.replays, "large_replays": args.large_replays, "repeats": args.repeats, "rows": []}
    g = torch.Generator().manual_seed(0)
    for s in (int(v) for v in args.shapes.split(",")):
        n, j, locality, is_large = SHAPES[s]
        k = metric.default_neighbors(locality, j)
        mo, mi = torch.rand(n, 2, generator=g).cuda(), torch.rand(j, 2, generator=g).cuda()
        builders = {
            "torch": lambda: metric.knn_lists(metric.sqdist_euclid, mo, mi, k, locality=locality),
            "rows": lambda: metric.knn_lists(metric.sqdist_euclid, mo, mi, k, locality=locality, select="hip"),
            "box": lambda: metric.knn_lists_box(mo, mi, k, locality=locality),
        }
        graphs, lists = {}, {}
        for name, fn in builders.items():
            graph, lists[name] = _capture(fn)
            graphs[name] = graph.replay
        form = ops.knn_last_form()
        replays = args.large_replays if is_large else args.replays
        res = _median_us(graphs, replays, args.repeats)
        ref = lists["torch"].idx.sort(-1).values
        for name, (us, blocks) in res.items():
            same = (lists[name].idx.sort(-1).values == ref).all(-1).float().mean()
            out["rows"].append({"n_out": n, "n_in": j, "locality": locality, "k": k, "builder": name, "replays": replays,
                                "us_per_build": round(us, 1), "blocks_us": blocks, "cut_rows": int(lists[name].cut_rows),
                                "rows_with_torch_key_set": round(float(same), 6), "knn_form": form if name != "torch" else None})
        del graphs, lists, mo, mi
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
