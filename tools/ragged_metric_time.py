#!/usr/bin/env python3
"""What a training step on ragged clouds costs through the any-metric stack, beside the Euclidean stack, in ONE process.

    python tools/ragged_metric_time.py [--replays 50] [--repeats 9] [--hid 256] [--blocks 4]

Two captured training steps (engine.TrainStep: forward, the ragged loss, backward; no optimizer) on the same Elasticity-shaped
batch - b = 10 clouds padded to 972 points, lengths uniform in [486, 972], 256 latent points shared by the batch, locality 0.02:
  metric   metric.pit_metric(neighbors="auto", builder="hip") with sqdist_euclid: per step the neighbour lists of the down and up
           layers from pit_knn_box_ragged, the listed distances recomputed by torch, the layers on pit_distlist_*_ragged_*, the
           processor on dense distance matrices (pit_distmat_*)
  latent   tasks.pit_cloud_latent: the Euclidean ragged kernels (pit_ragged.hip) and the batch-free processor
The two are different code paths of the same function class (per-sample clouds, one shared latent mesh); their weights differ
(pit_metric prepends the coordinates itself), so only the times are compared, not the numbers.

After a warm-up block the blocks of bare replays alternate between the two graphs, one synchronisation per block; every figure
is the median block over `--repeats`, divided by the replays.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
from timeit import default_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, WIDTH, LATENT, LOCALITY = 10, 972, 256, 0.02


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--hid", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=4)
    args = ap.parse_args()
    import torch
    from position_induced_transformer_amd import engine, metric, tasks
    if not torch.cuda.is_available():
        raise SystemExit("tools/ragged_metric_time.py measures on the HIP device; none found")
    g = torch.Generator().manual_seed(0)
    lengths = torch.randint(WIDTH // 2, WIDTH + 1, (BATCH,), generator=g).tolist()
    mesh, func, target, _ = tasks.ragged_clouds(lengths, WIDTH, seed=1, device="cuda")
    ltt = torch.rand(LATENT, 2, generator=g).cuda()                     # (on the device: a captured step cannot copy it there)
    torch.manual_seed(0)
    models = {
        "metric": metric.pit_metric(2, 1, 1, args.hid, 2, args.blocks, ltt, LOCALITY, LOCALITY, neighbors="auto", builder="hip").cuda(),
        "latent": tasks.pit_cloud_latent(2, 3, 1, args.hid, 2, args.blocks, ltt, LOCALITY, LOCALITY).cuda(),
    }
    inputs = {"metric": func, "latent": torch.cat((mesh, func), -1)}
    steps = {}
    for name, model in models.items():
        steps[name] = engine.TrainStep(model, (mesh, inputs[name], mesh, target), 1, 2, len_in=lengths)
        steps[name].capture(warmup=2)
    times = {name: [] for name in steps}
    for rep in range(args.repeats + 1):                                  # block 0 is the warm-up
        for name, step in steps.items():
            torch.cuda.synchronize()
            t0 = default_timer()
            for _ in range(args.replays):
                step.replay()
            torch.cuda.synchronize()
            if rep:
                times[name].append(default_timer() - t0)
    out = {"batch": BATCH, "width": WIDTH, "latent_points": LATENT, "locality": LOCALITY, "hid": args.hid, "blocks": args.blocks,
           "lengths": lengths, "replays": args.replays, "repeats": args.repeats, "neighbors": metric.default_neighbors(LOCALITY, WIDTH)}
    for name, t in times.items():
        out[name] = {"us_per_step": round(1e6 * statistics.median(t) / args.replays, 1),
                     "blocks_us": [round(1e6 * v / args.replays, 1) for v in t], "loss": float(steps[name].loss)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
