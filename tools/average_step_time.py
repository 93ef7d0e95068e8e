#!/usr/bin/env python3
"""Per-replay time of the captured Darcy b = 8 training step (43^2, fp32: the README headline's step) with ddp.GuardedAdam and
with ddp.AveragedAdam, in ONE process.

    python tools/average_step_time.py [--replays 200] [--repeats 9] [--average ema|equal]

Two models from one seed, each captured with its optimizer (zero_grads=True, as bench.py builds its step; both clip at --clip).
The two graphs hold the same launches: the averaged step's second optimizer launch also reads and writes the average, n floats
each way.  After a warm-up block the blocks of `--replays` bare replays alternate between the two steps, one synchronisation
per block; the figure is the median block over `--repeats`, divided by the replays.  The GuardedAdam figure is the control.
Also timed: one `with opt.averaged():` round trip (two pit_exchange_words launches) in blocks of its own.  Prints one JSON line.

    rocprofv3 --kernel-trace --stats -- python tools/average_step_time.py

gives the two instances' own times (adam_step_guarded_kernel<> and adam_step_guarded_kernel<avg_args>) and
exchange_words_kernel's in the kernel statistics of the trace."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
from timeit import default_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _example():
    spec = importlib.util.spec_from_file_location("train_darcy_synthetic", os.path.join(ROOT, "examples", "train_darcy_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--average", choices=("ema", "equal"), default="ema")
    args = ap.parse_args()
    import torch
    from position_induced_transformer_amd.ddp import AveragedAdam, FlatGradients, GuardedAdam
    from position_induced_transformer_amd.engine import TrainStep
    from position_induced_transformer_amd.utils import PixelWiseNormalization
    ex = _example()
    s = 43
    torch.manual_seed(0)
    x = torch.randn(args.batch, s, s, 1)
    k = torch.ones(1, 1, 5, 5) / 25.0
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), k, padding=2).permute(0, 2, 3, 1).contiguous()
    mesh, mesh_ltt = ex.grid(s), ex.grid(16)
    total = (args.repeats + 2) * args.replays
    steps = {}
    for name in ("guarded", "averaged"):
        torch.manual_seed(1)
        model = ex.pit_darcy(2, 1, 1, 64, 2, 4, mesh_ltt, 0.02, 0.02).cuda()
        normalizer = PixelWiseNormalization(y)
        normalizer.cuda()
        flat = FlatGradients(model.parameters(), flatten_params=True)
        kw = dict(lr=1e-3, cosine_t_max=total, zero_grads=True, max_grad_norm=args.clip)
        if name == "guarded":
            opt = GuardedAdam(flat, **kw)
        else:
            opt = AveragedAdam(flat, average=args.average, average_decay=0.999, **kw)
        step = TrainStep(model, (mesh, x.cuda(), mesh, y.cuda()), 1, 2, pred_affine=normalizer.affine(), optimizer=opt, flat=flat)
        step.capture()
        steps[name] = step
    times = {name: [] for name in steps}
    for rep in range(args.repeats + 1):                               # (block 0 of each step is the warm-up)
        for name, step in steps.items():
            torch.cuda.synchronize()
            t0 = default_timer()
            for _ in range(args.replays):
                step.replay()
            torch.cuda.synchronize()
            if rep:
                times[name].append(default_timer() - t0)
    out = {"batch": args.batch, "replays": args.replays, "repeats": args.repeats, "average": args.average,
           "n_params": int(steps["guarded"].flat.flat.numel())}
    for name in steps:
        out[name + "_us"] = 1e6 * statistics.median(times[name]) / args.replays
        out[name + "_blocks_us"] = [round(1e6 * t / args.replays, 2) for t in times[name]]
        out[name + "_loss"] = float(steps[name].loss)
    out["averaged_minus_guarded_us"] = out["averaged_us"] - out["guarded_us"]
    same = all(torch.equal(a, b) for a, b in zip(steps["guarded"].model.parameters(), steps["averaged"].model.parameters()))
    out["same_parameter_bits"] = bool(same)                           # (only in the reproducible mode is this promised)
    opt = steps["averaged"].optimizer
    swaps = []
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = default_timer()
        for _ in range(args.replays):
            with opt.averaged():
                pass
        torch.cuda.synchronize()
        if rep:
            swaps.append(default_timer() - t0)
    out["swap_round_trip_us"] = 1e6 * statistics.median(swaps) / args.replays
    out["n_averaged"] = int(opt.n_averaged)
    health = steps["averaged"].health()
    out["health"] = {"calls": health.calls, "applied": health.applied, "skipped": health.skipped, "clipped": health.clipped,
                     "max_norm": health.max_norm, "mean_loss": health.mean_loss}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
