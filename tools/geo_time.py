#!/usr/bin/env python3
"""What building GEODESIC neighbour lists costs on the device (metric.knn_lists_geodesic, one launch of pit_geo_knn), in ONE
process, with metric.knn_lists_box at the same shapes beside it for scale.

    python tools/geo_time.py [--replays 100] [--large-replays 3] [--repeats 9] [--parts small,large,step]

The two builders compute DIFFERENT functions (path lengths on the cloud's 8-nearest-neighbour graph against straight-line
distances): no ratio is claimed.  Shapes, uniform points in the unit square:
  small   b = 10 clouds of 972 points, the graph of metric.knn_graph(g = 8) built once outside the timing, 256 latent points by
          ops.farthest_point_sample - the three forms of metric.pit_cloud_geodesic:
            down       256 sources, every vertex a key, locality 0.02 (k = default_neighbors)
            processor  256 sources, the 256 latent points as keys, k = 64
            up         972 sources, the 256 latent points as keys, locality 0.02
  large   one cloud of 50 000 vertices, every vertex a source and a key, k = 32
  step    the captured training step (engine.TrainStep) of metric.pit_cloud_geodesic at the Elasticity shape (batch 10, 972 points,
          44 input channels, hid 256, 2 heads, 4 blocks, localities 0.02) with 256 latent points: graph build, sampling, the three
          list builds, forward, loss, backward.
Every build is captured into a hipGraph of its own (the search, the int64 keys, the squared lengths and the three counts).  After a
warm-up block the blocks of bare replays alternate between the graphs of a shape, one synchronisation per block; every figure is
the median block over `--repeats`, divided by the replays.  Also reported: truncated / short / cut rows.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from knn_time import _capture, _median_us  # noqa: E402


def _row(shape, name, k, us, blocks, replays, lists):
    row = {"shape": shape, "builder": name, "k": k, "replays": replays, "us_per_build": round(us, 1), "blocks_us": blocks,
           "cut_rows": int(lists.cut_rows)}
    if hasattr(lists, "truncated_rows"):
        row.update(truncated_rows=int(lists.truncated_rows), short_rows=int(lists.short_rows))
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--large-replays", type=int, default=3, help="replays per block at 50 000 vertices")
    ap.add_argument("--step-replays", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--parts", default="small,large,step")
    args = ap.parse_args()
    import torch
    from position_induced_transformer_amd import engine, metric, ops
    if not torch.cuda.is_available():
        raise SystemExit("tools/geo_time.py measures on the HIP device; none found")
    parts = args.parts.split(",")
    out = {"replays": args.replays, "large_replays": args.large_replays, "step_replays": args.step_replays, "repeats": args.repeats,
           "rows": []}
    g = torch.Generator().manual_seed(0)
    if "small" in parts:
        b, n, m, q = 10, 972, 256, 0.02
        pts = torch.rand(b, n, 2, generator=g).cuda()
        adj, w = metric.knn_graph(pts, 8)
        latent = ops.farthest_point_sample(pts, m)
        key_of = torch.full((b, n), -1, device="cuda", dtype=torch.int32)
        key_of.scatter_(1, latent.idx.long(), torch.arange(m, device="cuda", dtype=torch.int32).expand(b, m))
        k_down, k_up = metric.default_neighbors(q, n), metric.default_neighbors(q, m)
        forms = {
            "down": (k_down, lambda: metric.knn_lists_geodesic(adj, w, k_down, q, sources=latent.idx),
                     lambda: metric.knn_lists_box(latent.mesh, pts, k_down, locality=q)),
            "processor": (64, lambda: metric.knn_lists_geodesic(adj, w, 64, 1.0, sources=latent.idx, key_of=key_of, n_keys=m),
                          lambda: metric.knn_lists_box(latent.mesh, latent.mesh, 64)),
            "up": (k_up, lambda: metric.knn_lists_geodesic(adj, w, k_up, q, key_of=key_of, n_keys=m),
                   lambda: metric.knn_lists_box(pts, latent.mesh, k_up, locality=q)),
        }
        for form, (k, geo, box) in forms.items():
            graphs, lists = {}, {}
            for name, fn in (("geodesic", geo), ("box", box)):
                graph, lists[name] = _capture(fn)
                graphs[name] = graph.replay
            for name, (us, blocks) in _median_us(graphs, args.replays, args.repeats).items():
                out["rows"].append(_row(f"b10 V972 g8 {form}", name, k, us, blocks, args.replays, lists[name]))
    if "large" in parts:
        n, k = 50000, 32
        pts = torch.rand(n, 2, generator=g).cuda()
        adj, w = metric.knn_graph(pts, 8)
        graphs, lists = {}, {}
        for name, fn in (("geodesic", lambda: metric.knn_lists_geodesic(adj, w, k)), ("box", lambda: metric.knn_lists_box(pts, pts, k))):
            graph, lists[name] = _capture(fn)
            graphs[name] = graph.replay
        for name, (us, blocks) in _median_us(graphs, args.large_replays, args.repeats).items():
            out["rows"].append(_row("V50000 g8 all sources", name, k, us, blocks, args.large_replays, lists[name]))
        del graphs, lists
        torch.cuda.empty_cache()
    if "step" in parts:
        b, n = 10, 972
        torch.manual_seed(0)
        model = metric.pit_cloud_geodesic(2, 44, 1, 256, 2, 4, 256, 0.02, 0.02).cuda()
        mesh = torch.rand(b, n, 2, generator=g).cuda()
        func = torch.cat((mesh, (torch.rand(b, n, 42, generator=g) * 5 - 1).cuda()), -1)
        target = torch.randn(b, n, 1, generator=g).cuda()
        step = engine.TrainStep(model, (mesh, func, mesh, target), 1, 2, len_in=[n] * b)
        step.capture(warmup=2)
        us, blocks = _median_us({"step": step.replay}, args.step_replays, args.repeats)["step"]
        out["rows"].append({"shape": "b10 V972 elasticity step, 256 latent", "builder": "pit_cloud_geodesic TrainStep",
                            "replays": args.step_replays, "us_per_step": round(us, 1), "blocks_us": blocks, "loss": float(step.loss),
                            "truncated_rows": [int(l.truncated_rows) for l in model.last_lists],
                            "short_rows": [int(l.short_rows) for l in model.last_lists]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
