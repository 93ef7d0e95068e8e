#!/usr/bin/env python3
"""Training on point clouds of DIFFERENT sizes with one captured hipGraph: tasks.pit_cloud_latent (per-sample clouds on a
latent mesh shared by the batch) on synthetic ragged batches (tasks.ragged_clouds), engine.TrainStep with lengths and the fused
Adam (ddp.FlatAdam(zero_grads=True)).

    python examples/train_clouds_synthetic.py [--epochs 2] [--width 972] [--latent shared|fps:M|geo:M] [--feed] [--points M]
                                              [--clip NORM] [--ema DECAY] [--save PATH] [--resume PATH]

`--latent fps:M`: tasks.pit_cloud_fps instead - every cloud gets a latent mesh of its own, M of its points chosen by
farthest-point sampling (ops.farthest_point_sample: one launch inside the captured step, on the clouds the step was fed).
`--latent geo:M`: metric.pit_cloud_geodesic - M sampled latent points again, and all three attention stages on GEODESIC
neighbour lists (path lengths on each cloud's 8-nearest-neighbour graph, searched inside the captured step: ops.geo_knn).

The step is captured once for the padded width; every batch then brings its own point counts through
``set_batch(..., len_in=...)`` - the lengths live in a static device tensor the kernels read, so no replay waits for the
host.  The evaluation metric is the reference's for clouds, RelMaxNorm (train_elasticity.py:118), over the real points only.

After every epoch a held-out set of ragged batches is evaluated through one captured graph (engine.EvalStep with lengths): both
metrics add up on the device, the last batch is only partly filled (``n_valid``), and ``result()`` is the pass's one
synchronisation.

`--feed`: the clouds, their functions, targets and lengths stay on the device as one dataset, and the captured steps gather
their own shuffled batches from it (engine.DeviceFeed: meshes, functions, targets and the int32 lengths in one launch at the head
of the graph); an epoch is `steps_per_epoch` bare replays.

`--points M` (implies `--feed`): every training step sees a random subset of M points of each cloud, drawn by the feed's launch
(engine.DeviceFeed(subsample=True); a new subset per cloud in every epoch, the same one for mesh, function and target).  When M
fits the shortest cloud of the dataset the step is built WITHOUT lengths - a rectangular batch on the dense per-sample kernels -
otherwise with lengths, which then receive min(M, length).  The per-epoch evaluation runs on the full clouds, unchanged: the
model does not depend on the discretisation, so the subset is an estimate of the same loss at a fraction of the cost.

`--clip NORM`: the guarded step (ddp.GuardedAdam) instead of FlatAdam - the gradient's global norm clipped at NORM, updates with
a non-finite gradient skipped, and the epoch's `step.health()` line printed (one read of the device state per epoch).

`--ema DECAY`: ddp.AveragedAdam - the guarded step also keeps an exponential average of the weights, in the same two launches.
Every epoch is then evaluated twice through the SAME captured evaluation graph, on the live weights and, under
`with opt.averaged():`, on the average (the two buffers change places; nothing is captured again), and both errors are printed.

`--save PATH` writes `step.state_dict()` - model, optimizer (moments, counters, health slots, average) and the feed's position -
at the end of every epoch; `--resume PATH` loads it AFTER the capture (whose warm-up passes move the optimizer) and goes on at
the saved position (same `--epochs`: the schedule's length is part of the state, and `load_state_dict` refuses another).  PATH may
contain `{epoch}` to keep every epoch's file.  The position of a run is its feed's cursor, so both imply `--feed`."""
import argparse
import os
import sys
from timeit import default_timer

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from position_induced_transformer_amd import tasks  # noqa: E402
from position_induced_transformer_amd.ddp import AveragedAdam, FlatAdam, FlatGradients, GuardedAdam  # noqa: E402
from position_induced_transformer_amd.engine import DeviceFeed, EvalStep, TrainStep  # noqa: E402
from position_induced_transformer_amd.utils import RelMaxNorm, count_params  # noqa: E402


def batches(n_batches, batch, width, seed):
    """Synthetic "dataset": ragged batches whose clouds have between width / 2 and width points."""
    g = torch.Generator().manual_seed(seed)
    for i in range(n_batches):
        lengths = torch.randint(width // 2, width + 1, (batch,), generator=g).tolist()
        yield tasks.ragged_clouds(lengths, width, seed=seed * 1000 + i, device="cuda") + (lengths,)


def dataset(parts, last_rows=None):
    """The batches of ``parts`` as one dataset on the device (the last one cut to ``last_rows`` clouds): the fields of a feed."""
    parts = list(parts)
    rows = [len(p[0]) for p in parts[:-1]] + [last_rows or len(parts[-1][0])]
    cat = [torch.cat([p[k][:r] for p, r in zip(parts, rows)]).contiguous() for k in range(4)]
    return {"mesh_in": cat[0], "func_in": cat[1], "target": cat[2], "len_in": cat[3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--nbatches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--width", type=int, default=972)
    ap.add_argument("--hid", type=int, default=64)
    ap.add_argument("--latent", default="shared", metavar="shared|fps:M|geo:M",
                    help="the latent mesh: one 16 x 16 grid shared by the batch, or M points of each cloud by farthest-point sampling "
                         "(geo: with geodesic neighbour lists in every attention stage)")
    ap.add_argument("--feed", action="store_true", help="device-resident data feed inside the captured steps")
    ap.add_argument("--points", type=int, default=None, metavar="M",
                    help="train on a random subset of M points of each cloud, drawn inside the captured step (implies --feed)")
    ap.add_argument("--clip", type=float, default=None, metavar="NORM",
                    help="clip the gradient's global norm and skip non-finite updates inside the captured step")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="keep an exponential average of the weights inside the guarded step and evaluate it too")
    ap.add_argument("--save", default=None, metavar="PATH", help="write step.state_dict() after every epoch (implies --feed)")
    ap.add_argument("--resume", default=None, metavar="PATH", help="load a saved state after the capture and go on (implies --feed)")
    args = ap.parse_args()
    args.feed = args.feed or args.save is not None or args.resume is not None or args.points is not None
    if args.points is not None and not 1 <= args.points <= args.width:
        ap.error(f"--points {args.points}: 1 <= M <= --width")
    torch.manual_seed(0)
    if args.latent == "shared":
        mesh_ltt = tasks.grid_mesh_2d(16, True, "cuda").reshape(-1, 2)
        model = tasks.pit_cloud_latent(2, 1, 1, args.hid, 2, 4, mesh_ltt, 0.02, 0.02).cuda()
    elif args.latent.startswith("fps:") and args.latent[4:].isdigit() and 1 <= int(args.latent[4:]) <= args.width:
        model = tasks.pit_cloud_fps(2, 1, 1, args.hid, 2, 4, int(args.latent[4:]), 0.02, 0.02).cuda()
    elif args.latent.startswith("geo:") and args.latent[4:].isdigit() and 1 <= int(args.latent[4:]) <= args.width // 2:
        from position_induced_transformer_amd import metric
        model = metric.pit_cloud_geodesic(2, 1, 1, args.hid, 2, 4, int(args.latent[4:]), 0.02, 0.02).cuda()
    else:
        ap.error(f"--latent {args.latent}: 'shared', 'fps:M' with 1 <= M <= --width or 'geo:M' with 1 <= M <= --width / 2")
    print("parameters:", count_params(model))
    iterations = args.epochs * args.nbatches
    flat = FlatGradients(model.parameters(), flatten_params=True)
    guarded = args.clip is not None or args.ema is not None
    if args.ema is not None:
        opt = AveragedAdam(flat, lr=1e-3, cosine_t_max=iterations, zero_grads=True, max_grad_norm=args.clip, average="ema",
                           average_decay=args.ema)
    elif guarded:
        opt = GuardedAdam(flat, lr=1e-3, cosine_t_max=iterations, zero_grads=True, max_grad_norm=args.clip)
    else:
        opt = FlatAdam(flat, lr=1e-3, cosine_t_max=iterations, zero_grads=True)
    # the static buffers of the captured step: the first batch, the query points are the clouds themselves
    mesh, func, target, lens, _ = next(batches(1, args.batch, args.width, seed=1))
    if args.points is None:
        step = TrainStep(model, (mesh, func, mesh, target), 1, 2, optimizer=opt, flat=flat, len_in=lens)
        if args.feed:
            feed = DeviceFeed(step, dataset(batches(args.nbatches, args.batch, args.width, seed=2)), shuffle=True, seed=0)
    else:
        # static buffers of M points; the feed fills them with a subset of every cloud.  Lengths only if a cloud is shorter
        data = dataset(batches(args.nbatches, args.batch, args.width, seed=2))
        shortest = int(data["len_in"].min())
        cut = mesh[:, :args.points].contiguous()
        kw = {"len_in": [args.points] * args.batch} if shortest < args.points else {}
        step = TrainStep(model, (cut, func[:, :args.points].contiguous(), cut, target[:, :args.points].contiguous()), 1, 2,
                         optimizer=opt, flat=flat, **kw)
        feed = DeviceFeed(step, data, shuffle=True, seed=0, subsample=True)
        print(f"training on {args.points} of up to {args.width} points per cloud (shortest cloud {shortest}): a step "
              f"{'with' if kw else 'without'} lengths")
    step.capture()
    if guarded:
        step.health(reset=True)                                      # (the warm-up passes of the capture are not this epoch's)
    first_epoch = skip = 0
    if args.resume is not None:                                      # build, capture, THEN load: the load overwrites the warm-up
        step.load_state_dict(torch.load(args.resume, weights_only=True))
        first_epoch, skip = divmod(int(feed.cursor), feed.steps_per_epoch)
        print(f"resumed {args.resume} at step {int(feed.cursor)} (epoch {first_epoch})")
    metric = RelMaxNorm(1)
    # the held-out set: nbatches // 4 + 1 batches, the last of which holds batch // 2 clouds only
    held_out = list(batches(args.nbatches // 4 + 1, args.batch, args.width, seed=99))
    last_valid = max(1, args.batch // 2)
    n_test = (len(held_out) - 1) * args.batch + last_valid
    emesh = mesh.clone()                                             # (static buffers of its own; queries = the clouds themselves)
    evaluate = EvalStep(model, (emesh, func.clone(), emesh, target.clone()), 1, 2, capacity=n_test, len_in=lens.clone())
    if args.feed:
        test_feed = DeviceFeed(evaluate, dataset(held_out, last_valid), shuffle=False, drop_last=False)
    evaluate.capture()

    def run_eval():
        evaluate.reset()                                             # (also sends an attached feed back to its first batch)
        if args.feed:
            for _ in range(test_feed.steps_per_epoch):               # (the feed writes n_valid for the last batch)
                evaluate.replay()
        else:
            for i, (m, f, t, _, lengths) in enumerate(held_out):
                evaluate.set_batch(f, t, mesh_in=m, len_in=lengths, n_valid=last_valid if i == len(held_out) - 1 else args.batch)
                evaluate.replay()
        return evaluate.result()                                     # the pass's only synchronisation

    for ep in range(first_epoch, args.epochs):
        t1 = default_timer()
        train_l2 = torch.zeros((), device="cuda")
        train_max = torch.zeros((), device="cuda")
        if args.feed:
            for _ in range(feed.steps_per_epoch - (skip if ep == first_epoch else 0)):
                step.replay()                                        # the feed's launch is the first of the graph
                train_l2 += step.loss
                train_max += metric(step.target, step.out, step.len_in)
        else:
            for m, f, t, _, lengths in batches(args.nbatches, args.batch, args.width, seed=2 + ep):
                step.set_batch(f, t, mesh_in=m, len_in=lengths)      # new clouds, new sizes, the same graph
                step.replay()
                train_l2 += step.loss
                train_max += metric(step.target, step.out, step.len_in)      # the prediction of the replay, real points only
        torch.cuda.synchronize()
        t2 = default_timer()
        n = args.nbatches * args.batch
        test = run_eval()
        print(ep, f"{t2 - t1:.3f}s", "rel-L2", float(train_l2) / n, "rel-max", float(train_max) / n,
              "| test rel-L2", test.rel_lp / test.count, "rel-max", test.rel_max / test.count, "samples", test.count)
        if args.ema is not None:
            with opt.averaged():                                     # the same graph reads the average where the weights live
                avg = run_eval()
            print("   averaged weights (%d updates): test rel-L2" % int(opt.n_averaged), avg.rel_lp / avg.count, "rel-max",
                  avg.rel_max / avg.count)
        if guarded:
            h = step.health(reset=True)
            print(f"   guard: applied {h.applied} skipped {h.skipped} clipped {h.clipped} of {h.calls}; largest norm {h.max_norm:.4g}, "
                  f"last {h.norm:.4g} (coef {h.coef:.4g}); train loss per sample {h.mean_loss / args.batch:.6g} "
                  f"({h.nonfinite_loss} not finite)")
        if args.save is not None:
            torch.save(step.state_dict(), args.save.format(epoch=ep))


if __name__ == "__main__":
    main()
