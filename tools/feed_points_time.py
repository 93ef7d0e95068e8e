#!/usr/bin/env python3
"""What a random subset of each cloud's points costs when the feed draws it (ops.batch_feed_points /
engine.DeviceFeed(subsample=True)), in ONE process.

    python tools/feed_points_time.py [--replays 200] [--repeats 9] [--samples 200]
    rocprofv3 --kernel-trace --stats -- python tools/feed_points_time.py --kernels [--launches 200]

1. The launch alone, against pit_batch_feed moving the SAME number of destination bytes (a dataset whose rows are as wide as the
   subset): b=10 n=972 m=486 and b=4 n=16384 m=4096, Elasticity's 44 + 2 + 1 words per point (function, mesh, target; one
   cloud).  `--kernels` only issues the launches - `--launches` of each after 20 warm-up launches - and prints the bytes each
   moves, for a kernel trace: the two shapes run different instances (256 and 1024 threads) of batch_feed_points_kernel and
   batch_feed_kernel, so the trace's per-kernel averages are per shape; GB/s = 2 x destination bytes / time (every word is read
   once and written once).  Without `--kernels` each launch is captured alone into a hipGraph and timed by replays (launch
   overhead included: what a captured step pays at its head).
2. Three captured training steps at the Elasticity shape of tools/fps_time.py - tasks.pit_cloud_fps, 44 input channels, hid 128,
   2 heads, 4 blocks, n_latent 256, fp32, ddp.FlatAdam(zero_grads=True) in the graph, batch 10, clouds of width 972 with lengths
   uniform in [486, 972]:
     (a) the plain feed and a step with len_in at width 972 (what the package could do before);
     (b) the subsampling feed to m = 486 and a step WITHOUT lengths;
     (c) the subsampling feed to m = 486 and a step with lengths.
   (b) and (c) estimate the loss on half the points of every cloud: this is a cost table, not a speed-up of one computation.

After a warm-up block the blocks of `--replays` bare replays alternate between the graphs, one synchronisation per block; every
figure is the median block over `--repeats`, divided by the replays.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fps_time import _capture, _median_us  # noqa: E402

SHAPES = ((10, 972, 486), (4, 16384, 4096))                          # batch, n, m
WORDS = (44, 2, 1)                                                   # function, mesh, target
SAMPLES = 40                                                         # clouds in the datasets of part 1


def _launches():
    """{name: (launch, destination bytes)} for the subsampling and the plain feed at every shape."""
    import torch
    from position_induced_transformer_amd import ops
    g = torch.Generator().manual_seed(0)
    out, keep = {}, []
    for b, n, m in SHAPES:
        wide = [torch.rand(SAMPLES, n, w, generator=g).cuda() for w in WORDS]
        narrow = [t[:, :m].contiguous() for t in wide]
        nbytes = 4 * b * m * sum(WORDS)
        for name, src in (("points", wide), ("plain", narrow)):
            dst = [torch.zeros(b, m, w, device="cuda") for w in WORDS]
            state = ops.new_feed_state("cuda")
            if name == "points":
                def launch(src=src, dst=dst, state=state):
                    ops.batch_feed_points(src, dst, [1, 1, 1], state, seed=3)
            else:
                def launch(src=src, dst=dst, state=state):
                    ops.batch_feed(src, dst, state, seed=3)
            keep.append((src, dst, state))
            out[f"{name}_b{b}_n{n}_m{m}"] = (launch, nbytes)
    return out, keep


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--samples", type=int, default=200, help="clouds in the dataset of the captured steps")
    ap.add_argument("--kernels", action="store_true", help="only issue the feed launches (for a kernel trace)")
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    import torch
    from position_induced_transformer_amd import tasks
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    launches, keep = _launches()
    if args.kernels:
        for name, (launch, nbytes) in launches.items():
            for _ in range(20 + args.launches):
                launch()
            torch.cuda.synchronize()
        print(json.dumps({"launches": args.launches, "warmup": 20,
                          "destination_bytes": {name: nbytes for name, (_, nbytes) in launches.items()}}))
        return
    out = {"replays": args.replays, "repeats": args.repeats, "launch": {}}
    graphs = {name: _capture(launch)[0] for name, (launch, _) in launches.items()}
    for name, (us, blocks) in _median_us({k: v.replay for k, v in graphs.items()}, args.replays, args.repeats).items():
        nbytes = launches[name][1]
        out["launch"][name] = {"us": round(us, 2), "destination_bytes": nbytes, "GBps": round(2 * nbytes / us / 1e3, 1),
                               "blocks_us": blocks}
    # the captured steps
    b, n, m, N = 10, 972, 486, args.samples
    g = torch.Generator().manual_seed(1)
    lengths = torch.randint(m, n + 1, (N,), generator=g)
    xy = torch.rand(N, n, 2, generator=g)
    feats = torch.cat((xy, torch.rand(N, n, 42, generator=g) * 5 - 1), -1)     # (tasks.make_task("elasticity"))
    target = torch.randn(N, n, 1, generator=g)
    for i, length in enumerate(lengths.tolist()):                     # padding that would show if it were read
        xy[i, length:] = feats[i, length:] = target[i, length:] = float("nan")
    data = {"mesh_in": xy.cuda(), "func_in": feats.cuda(), "target": target.cuda(), "len_in": lengths.to(torch.int32).cuda()}
    total = (args.repeats + 2) * args.replays
    steps = {}
    for name, width, lens, sub in (("a_plain_len972", n, True, False), ("b_sub486", m, False, True), ("c_sub486_len", m, True, True)):
        torch.manual_seed(1)
        model = tasks.pit_cloud_fps(2, 44, 1, 128, 2, 4, 256, 0.02, 0.02).cuda()
        flat = FlatGradients(model.parameters(), flatten_params=True)
        opt = FlatAdam(flat, lr=1e-3, cosine_t_max=total, zero_grads=True)
        mesh = torch.zeros(b, width, 2, device="cuda")
        batch = (mesh, torch.zeros(b, width, 44, device="cuda"), mesh, torch.zeros(b, width, 1, device="cuda"))
        step = TrainStep(model, batch, 1, 2, optimizer=opt, flat=flat, **({"len_in": [width] * b} if lens else {}))
        DeviceFeed(step, data, seed=0, subsample=sub)
        step.capture()
        steps[name] = step
    res = _median_us({name: step.replay for name, step in steps.items()}, args.replays, args.repeats)
    out["step"] = {"batch": b, "width": n, "points": m, "hid": 128, "n_latent": 256, "samples": N}
    for name, (us, blocks) in res.items():
        out["step"][name + "_ms"] = round(us / 1e3, 4)
        out["step"][name + "_blocks_ms"] = [round(v / 1e3, 4) for v in blocks]
        out["step"][name + "_loss"] = float(steps[name].loss)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
