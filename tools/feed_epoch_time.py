#!/usr/bin/env python3
"""Wall time of a training epoch with and without the device-resident data feed (engine.DeviceFeed), and a driver for the
kernel-time measurement of the feed's launch.

    python tools/feed_epoch_time.py [--ntrain 1024] [--batch 8] [--epochs 5]

runs, each in a FRESH child process, the epoch loop of examples/train_darcy_synthetic.py (Darcy 43^2, fp32, Adam in the graph):
  graph   the `--graph` loop as the example has it: DataLoader (host shuffle and collate), two `.cuda()` copies, `set_batch`,
          `replay`, `train_l2 += step.loss`
  feed    the `--feed` loop: `replay`, `train_l2 += step.loss`
  bare    `replay` alone with the feed attached (what an epoch costs when nothing but the graph is launched)
  plain   `replay` alone WITHOUT a feed, on one unchanging batch: the floor of this loop, the graph less the feed's launch
One warm-up epoch, then the median of `--epochs` epochs, one synchronisation per epoch.  Prints one JSON line.

    rocprofv3 --kernel-trace --stats -- python tools/feed_epoch_time.py --kernels darcy        (or: vorticity)

launches `batch_feed_kernel` 200 times at Darcy b = 8 (two fields of 7396-byte rows out of 1024 samples) or at Vorticity 64^2
b = 20 (a history of 10 and 20 targets: rows of 163840 and 327680 bytes out of 200 samples), and after them 200 times the two
`copy_` launches of `set_batch` at the same shape; the kernel statistics of the trace are the measurement (one shape per run,
so that they are that shape's)."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
from timeit import default_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _example():
    spec = importlib.util.spec_from_file_location("train_darcy_synthetic", os.path.join(ROOT, "examples", "train_darcy_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def child(mode: str, ntrain: int, batch: int, epochs: int) -> None:
    import torch
    from position_induced_transformer_amd.ddp import FlatAdam, FlatGradients
    from position_induced_transformer_amd.engine import DeviceFeed, TrainStep
    from position_induced_transformer_amd.utils import PixelWiseNormalization
    ex = _example()
    torch.manual_seed(0)
    s = 43
    x_train = torch.randn(ntrain, s, s, 1)
    k = torch.ones(1, 1, 5, 5) / 25.0
    y_train = torch.nn.functional.conv2d(x_train.permute(0, 3, 1, 2), k, padding=2).permute(0, 2, 3, 1).contiguous()
    x_train = PixelWiseNormalization(x_train).normalize(x_train)
    y_normalizer = PixelWiseNormalization(y_train)
    mesh, mesh_ltt = ex.grid(s), ex.grid(16)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x_train, y_train), batch_size=batch, shuffle=True,
                                         drop_last=True)
    model = ex.pit_darcy(2, 1, 1, 64, 2, 4, mesh_ltt, 0.02, 0.02).cuda()
    y_normalizer.cuda()
    flat = FlatGradients(model.parameters(), flatten_params=True)
    opt = FlatAdam(flat, lr=1e-3, cosine_t_max=(epochs + 1) * (ntrain // batch))
    x0, y0 = next(iter(loader))
    step = TrainStep(model, (mesh, x0.cuda(), mesh, y0.cuda()), 1, 2, pred_affine=y_normalizer.affine(), optimizer=opt, flat=flat)
    feed = None
    if mode in ("feed", "bare"):
        feed = DeviceFeed(step, {"func_in": x_train.cuda(), "target": y_train.cuda()}, shuffle=True, seed=0)
    step.capture()
    times = []
    for ep in range(epochs + 1):
        torch.cuda.synchronize()
        t1 = default_timer()
        train_l2 = torch.zeros((), device="cuda")
        if mode == "graph":
            for x, y in loader:
                x, y = x.cuda(), y.cuda()
                step.set_batch(x, y)
                step.replay()
                train_l2 += step.loss
        elif mode == "feed":
            for _ in range(feed.steps_per_epoch):
                step.replay()
                train_l2 += step.loss
        else:
            for _ in range(ntrain // batch):
                step.replay()
        torch.cuda.synchronize()
        if ep:
            times.append(default_timer() - t1)
    steps = ntrain // batch
    print(json.dumps({"mode": mode, "steps": steps, "epoch_ms": 1e3 * statistics.median(times),
                      "step_ms": 1e3 * statistics.median(times) / steps, "epochs_ms": [round(1e3 * t, 3) for t in times],
                      "loss": float(step.loss)}))


CHILD_TIMEOUT_S = 120


SHAPES = {"darcy": (1024, 8, ((43, 43, 1), (43, 43, 1))), "vorticity": (200, 20, ((64, 64, 10), (64, 64, 20)))}


def kernels(shape: str, launches: int = 200) -> None:
    import torch
    from position_induced_transformer_amd import ops
    n, batch, rows = SHAPES[shape]
    src = [torch.randn(n, *r, device="cuda") for r in rows]
    dst = [torch.zeros(batch, *r, device="cuda") for r in rows]
    new = [torch.randn(batch, *r, device="cuda") for r in rows]
    state = ops.new_feed_state("cuda")
    indices = torch.zeros(batch, dtype=torch.int32, device="cuda")
    for _ in range(launches):
        ops.batch_feed(src, dst, state, 0, 1, True, True, None, 0, indices, None)
    torch.cuda.synchronize()
    for _ in range(launches):                                         # the two copies of set_batch at the same shape
        dst[0].copy_(new[0])
        dst[1].copy_(new[1])
    torch.cuda.synchronize()
    nbytes = sum(d.numel() * 4 for d in dst)
    print(json.dumps({"shape": shape, "bytes_read_once_written_once": 2 * nbytes, "launches": launches}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntrain", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--child", choices=("graph", "feed", "bare", "plain"))
    ap.add_argument("--kernels", choices=tuple(SHAPES))
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    if args.child:
        return child(args.child, args.ntrain, args.batch, args.epochs)
    out = {}
    for mode in ("graph", "feed", "bare", "plain"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--ntrain", str(args.ntrain), "--batch", str(args.batch),
               "--epochs", str(args.epochs)]
        # a child builds the model, captures and runs epochs + 1 epochs of ~30 ms: seconds; a hung child must not hang the tool
        done = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S + 2 * args.epochs)
        out[mode] = json.loads(done.stdout.strip().splitlines()[-1])
    out["graph_over_feed"] = out["graph"]["epoch_ms"] / out["feed"]["epoch_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
