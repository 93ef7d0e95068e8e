#!/usr/bin/env python3
"""What farthest-point sampling costs on the device (ops.farthest_point_sample / tasks.pit_cloud_fps), in ONE process.

    python tools/fps_time.py [--replays 200] [--repeats 9] [--lengths]
    python tools/fps_time.py --large [--slices 0,512,2048] [--large-replays 50]

1. The sampler alone: one pit_fps launch captured into a hipGraph, at b=10 n=972 m=256, b=8 n=4096 m=512 and b=4 n=16384
   m=1024 (uniform clouds in the unit square) - microseconds per launch and nanoseconds per picked point (the launch is m
   dependent picks; the per-pick figure is the length of one iteration's critical path).
2. Two captured training steps at the Elasticity shape - b=10, 972 points, 44 input channels, hid 128, 2 heads, 4 blocks, fp32,
   ddp.FlatAdam(zero_grads=True) in the graph: tasks.pit_elasticity, whose latent mesh is the cloud itself, and
   tasks.pit_cloud_fps with --latent (default 256) sampled points.  The two models are DIFFERENT functions: the comparison states
   what each costs per step, not a speed-up of one computation.  `--lengths`: both steps on the ragged path (full-width lengths).

`--large`: the large sampler instead (ops.farthest_point_sample_large: one launch per pick, m kernel nodes in the graph), with m = 1024
and every slice size of `--slices` (0: the library's choice): at b=4 n=16384 BOTH samplers, alternating in blocks of `--replays`;
then the large sampler alone at n=65536 and n=262144, b=1 and b=4, in blocks of `--large-replays` (a sampling takes
milliseconds there).  Microseconds per sampling and per pick.

After a warm-up block the blocks of `--replays` bare replays alternate between the graphs, one synchronisation per block; every
figure is the median block over `--repeats`, divided by the replays.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
from timeit import default_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((10, 972, 256), (8, 4096, 512), (4, 16384, 1024))


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


LARGE_M = 1024
LARGE_BOTH = (4, 16384)
LARGE_ALONE = ((1, 65536), (4, 65536), (1, 262144), (4, 262144))


def large(args) -> dict:
    import torch
    from position_induced_transformer_amd import ops
    slices = [int(v) for v in args.slices.split(",")]
    out = {"replays": args.replays, "large_replays": args.large_replays, "repeats": args.repeats, "m": LARGE_M, "both": [], "large": []}
    g = torch.Generator().manual_seed(0)
    keep = []

    def rows(graphs, shapes, replays, dest):
        for (kind, b, n, sp), (us, blocks) in zip(shapes, _median_us(graphs, replays, args.repeats).values()):
            dest.append({"sampler": kind, "batch": b, "n": n, "slice_points": sp, "us_per_sampling": round(us, 1),
                         "us_per_pick": round(us / LARGE_M, 3), "blocks_us": blocks})

    b, n = LARGE_BOTH
    mesh = torch.rand(b, n, 2, generator=g).cuda()
    graph, res = _capture(lambda: ops.farthest_point_sample(mesh, LARGE_M))
    keep.append((mesh, res))
    graphs, shapes = {"small": graph.replay}, [("pit_fps", b, n, None)]
    for sp in slices:
        graph, res = _capture(lambda: ops.farthest_point_sample_large(mesh, LARGE_M, slice_points=sp))
        keep.append(res)
        assert torch.equal(res.idx, keep[0][1].idx)
        graphs[f"large_{sp}"] = graph.replay
        shapes.append(("pit_fps_large", b, n, sp))
    rows(graphs, shapes, args.replays, out["both"])
    graphs, shapes = {}, []
    for b, n in LARGE_ALONE:
        mesh = torch.rand(b, n, 2, generator=g).cuda()
        for sp in slices:
            graph, res = _capture(lambda: ops.farthest_point_sample_large(mesh, LARGE_M, slice_points=sp))
            keep.append((mesh, res))
            graphs[f"b{b}_n{n}_{sp}"] = graph.replay
            shapes.append(("pit_fps_large", b, n, sp))
    rows(graphs, shapes, args.large_replays, out["large"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--latent", type=int, default=256)
    ap.add_argument("--lengths", action="store_true", help="both training steps on the ragged path (full-width lengths)")
    ap.add_argument("--large", action="store_true", help="the large sampler (one launch per pick) instead")
    ap.add_argument("--slices", default="0", help="--large: comma-separated slice_points to time (0: the library's choice)")
    ap.add_argument("--large-replays", type=int, default=50, help="--large: replays per block at n = 65536 and 262144")
    args = ap.parse_args()
    if args.large:
        print(json.dumps(large(args)))
        return
    import torch
    from position_induced_transformer_amd import ops, tasks
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    from position_induced_transformer_amd.engine import TrainStep
    out = {"replays": args.replays, "repeats": args.repeats, "sampler": [], "lengths": bool(args.lengths)}
    g = torch.Generator().manual_seed(0)
    graphs, keep = {}, []
    for b, n, m in SHAPES:
        mesh = torch.rand(b, n, 2, generator=g).cuda()
        graph, res = _capture(lambda: ops.farthest_point_sample(mesh, m))
        keep.append((mesh, res))
        graphs[f"b{b}_n{n}_m{m}"] = graph.replay
    for (b, n, m), (name, (us, blocks)) in zip(SHAPES, _median_us(graphs, args.replays, args.repeats).items()):
        out["sampler"].append({"batch": b, "n": n, "m": m, "us_per_launch": round(us, 2), "ns_per_pick": round(1e3 * us / m, 1),
                               "blocks_us": blocks})
    total = (args.repeats + 2) * args.replays
    xy = torch.rand(10, 972, 2, generator=g)
    feats = torch.cat((xy, torch.rand(10, 972, 42, generator=g) * 5 - 1), -1).cuda()       # (tasks.make_task("elasticity"))
    xy, target = xy.cuda(), torch.randn(10, 972, 1, generator=g).cuda()
    steps = {}
    for name in ("elasticity", "cloud_fps"):
        torch.manual_seed(1)
        if name == "elasticity":
            model = tasks.pit_elasticity(2, 44, 1, 128, 2, 4, None, 0.02, 0.02).cuda()
        else:
            model = tasks.pit_cloud_fps(2, 44, 1, 128, 2, 4, args.latent, 0.02, 0.02).cuda()
        flat = FlatGradients(model.parameters(), flatten_params=True)
        opt = FlatAdam(flat, lr=1e-3, cosine_t_max=total, zero_grads=True)
        kw = {"len_in": [972] * 10} if args.lengths else {}
        step = TrainStep(model, (xy, feats, xy, target), 1, 2, optimizer=opt, flat=flat, **kw)
        step.capture()
        steps[name] = step
    res = _median_us({name: step.replay for name, step in steps.items()}, args.replays, args.repeats)
    out["step"] = {"batch": 10, "points": 972, "hid": 128, "n_latent": args.latent}
    for name, (us, blocks) in res.items():
        out["step"][name + "_ms"] = round(us / 1e3, 4)
        out["step"][name + "_blocks_ms"] = [round(v / 1e3, 4) for v in blocks]
        out["step"][name + "_loss"] = float(steps[name].loss)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
