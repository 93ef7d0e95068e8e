#!/usr/bin/env python3
"""The reference's Darcy training loop (train_darcy.py:62-150) on synthetic fields, written the
way the reference writes it - `from pit import *`, `class pit_darcy(pit_fixed)` with its own
forward, Adam + CosineAnnealingLR, RelLpNorm - but importing the MI355X modules instead.

    python examples/train_darcy_synthetic.py [--epochs 2] [--graph | --feed] [--clip NORM] [--ema DECAY]
                                             [--save PATH] [--resume PATH]

`--graph` replaces the inner loop by the hipGraph-captured step (engine.TrainStep) with the
fused Adam; without it the loop is literally the reference's eager loop.

After every epoch a held-out synthetic set is evaluated as train_darcy.py:136-144 does, through one captured
graph per batch (engine.EvalStep): the errors add up on the device, the last batch is only partly filled
(``n_valid``), and ``result()`` is the one synchronisation of the pass.

`--feed` (implies `--graph`) also keeps both datasets on the device and lets the captured steps fetch their own batches
(engine.DeviceFeed): an epoch is `steps_per_epoch` bare replays - no loader, no `.cuda()`, no `set_batch` - with the shuffle
done by the feed's keyed permutation, and the evaluation pass gets its `n_valid` from the feed.

`--clip NORM` (implies `--graph`) puts the guarded step in the graph (ddp.GuardedAdam): the gradient's global norm is clipped
at NORM, an update whose gradient is not finite is skipped, and the epoch's line of `step.health()` - steps applied, skipped and
clipped, the largest norm, the mean training loss from the device accumulator - is printed after each epoch.

`--ema DECAY` (implies `--graph`) uses ddp.AveragedAdam: the guarded step also keeps an exponential average of the weights, in the
same two launches.  Each epoch is then evaluated twice through the SAME captured evaluation graph - on the live weights and, under
`with opt.averaged():`, on the average (the two buffers change places in memory; nothing is captured again) - and both errors
are printed.

`--save PATH` writes `step.state_dict()` - model, optimizer (moments, counters, health slots, average) and the feed's position -
at the end of every epoch; `--resume PATH` loads it AFTER the capture (whose warm-up passes move the optimizer) and continues at
the saved position (same `--epochs`: the schedule's length is part of the state, and `load_state_dict` refuses another).  PATH may
contain `{epoch}` to keep every epoch's file.  The position of a run is its feed's cursor, so both imply `--feed`."""
import argparse
import os
import sys
from timeit import default_timer

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from position_induced_transformer_amd.pit import *      # noqa: F401,F403  (the reference does `from pit import *`)
from position_induced_transformer_amd.utils import *    # noqa: F401,F403


class pit_darcy(pit_fixed):                              # noqa: F405   train_darcy.py:25-59
    def forward(self, mesh_in, func_in, mesh_out):
        size = mesh_out.shape[:-1]
        mesh_in = mesh_in.reshape(-1, self.space_dim)
        func_in = func_in.reshape(func_in.shape[0], -1, self.in_dim)
        mesh_out = mesh_out.reshape(-1, self.space_dim)
        func_in = torch.cat((torch.tile(mesh_in.unsqueeze(0), [func_in.shape[0], 1, 1]), func_in), -1)  # noqa: F405
        func_ltt = self.encoder(mesh_in, func_in, self.mesh_ltt)
        func_ltt = self.processor(func_ltt, self.mesh_ltt)
        func_out = self.decoder(self.mesh_ltt, func_ltt, mesh_out)
        return func_out.reshape(func_in.shape[0], *size, self.out_dim)


def grid(s):
    m = np.vstack([xx.ravel() for xx in np.meshgrid(np.linspace(0, 1, s), np.linspace(0, 1, s))]).T  # noqa: F405
    return torch.tensor(m.reshape(s, s, 2), dtype=torch.float).cuda()  # noqa: F405


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--ntrain", type=int, default=256)
    ap.add_argument("--ntest", type=int, default=100)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--feed", action="store_true", help="device-resident data feed inside the captured steps (implies --graph)")
    ap.add_argument("--clip", type=float, default=None, metavar="NORM",
                    help="clip the gradient's global norm and skip non-finite updates inside the captured step (implies --graph)")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="keep an exponential average of the weights inside the guarded step and evaluate it too (implies --graph)")
    ap.add_argument("--save", default=None, metavar="PATH", help="write step.state_dict() after every epoch (implies --feed)")
    ap.add_argument("--resume", default=None, metavar="PATH", help="load a saved state after the capture and go on (implies --feed)")
    args = ap.parse_args()
    args.feed = args.feed or args.save is not None or args.resume is not None
    args.graph = args.graph or args.feed or args.clip is not None or args.ema is not None
    guarded = args.clip is not None or args.ema is not None
    torch.manual_seed(0)  # noqa: F405
    s = 43
    # synthetic "dataset": smooth random coefficient fields and a fixed smoothing of them as targets
    x_train = torch.randn(args.ntrain, s, s, 1)  # noqa: F405
    x_test = torch.randn(args.ntest, s, s, 1)  # noqa: F405
    k = torch.ones(1, 1, 5, 5) / 25.0  # noqa: F405
    y_train = torch.nn.functional.conv2d(x_train.permute(0, 3, 1, 2), k, padding=2).permute(0, 2, 3, 1)  # noqa: F405
    y_test = torch.nn.functional.conv2d(x_test.permute(0, 3, 1, 2), k, padding=2).permute(0, 2, 3, 1)  # noqa: F405
    x_normalizer = PixelWiseNormalization(x_train)  # noqa: F405
    x_train = x_normalizer.normalize(x_train)
    x_test = x_normalizer.normalize(x_test).cuda()
    y_test = y_test.cuda()
    y_normalizer = PixelWiseNormalization(y_train)  # noqa: F405
    mesh, mesh_ltt = grid(s), grid(16)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x_train, y_train),  # noqa: F405
                                         batch_size=args.batch, shuffle=True, drop_last=True)
    model = pit_darcy(2, 1, 1, 64, 2, 4, mesh_ltt, 0.02, 0.02).cuda()
    print("parameters:", count_params(model))  # noqa: F405
    iterations = args.epochs * (args.ntrain // args.batch)
    myloss = RelLpNorm(out_dim=1, p=2)  # noqa: F405
    y_normalizer.cuda()

    if args.graph:
        from position_induced_transformer_amd.ddp import AveragedAdam, FlatAdam, FlatGradients, GuardedAdam
        from position_induced_transformer_amd.engine import TrainStep
        flat = FlatGradients(model.parameters(), flatten_params=True)
        if args.ema is not None:
            opt = AveragedAdam(flat, lr=1e-3, cosine_t_max=iterations, max_grad_norm=args.clip, average="ema", average_decay=args.ema)
        elif guarded:
            opt = GuardedAdam(flat, lr=1e-3, cosine_t_max=iterations, max_grad_norm=args.clip)
        else:
            opt = FlatAdam(flat, lr=1e-3, cosine_t_max=iterations)
        x0, y0 = next(iter(loader))
        step = TrainStep(model, (mesh, x0.cuda(), mesh, y0.cuda()), 1, 2, pred_affine=y_normalizer.affine(),
                         optimizer=opt, flat=flat)
        if args.feed:
            from position_induced_transformer_amd.engine import DeviceFeed
            feed = DeviceFeed(step, {"func_in": x_train.cuda(), "target": y_train.cuda()}, shuffle=True, seed=0)
        step.capture()
        if guarded:
            step.health(reset=True)                                   # (the warm-up passes of the capture are not this epoch's)
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)  # noqa: F405
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=iterations)  # noqa: F405

    # the evaluation pass (built after FlatGradients re-homed the parameters: the graph reads them where they live now)
    from position_induced_transformer_amd.engine import EvalStep
    evaluate = EvalStep(model, (mesh, x_test[:args.batch].clone(), mesh, y_test[:args.batch].clone()), 1, 2,
                        pred_affine=y_normalizer.affine(), capacity=args.ntest)
    if args.feed:
        test_feed = DeviceFeed(evaluate, {"func_in": x_test, "target": y_test}, shuffle=False, drop_last=False)
    evaluate.capture()

    def run_eval():
        evaluate.reset()                                              # (also sends an attached feed back to its first batch)
        if args.feed:
            for _ in range(test_feed.steps_per_epoch):                # (the feed writes n_valid for the last batch)
                evaluate.replay()
        else:
            for i in range(0, args.ntest, args.batch):
                x, y = x_test[i:i + args.batch], y_test[i:i + args.batch]
                evaluate.set_batch(x, y, n_valid=x.shape[0])          # (the last batch brings fewer rows)
                evaluate.replay()
        return evaluate.result()                                      # the pass's only synchronisation

    first_epoch = skip = 0
    if args.resume is not None:                                       # build, capture, THEN load: the load overwrites the warm-up
        step.load_state_dict(torch.load(args.resume, weights_only=True))  # noqa: F405
        first_epoch, skip = divmod(int(feed.cursor), feed.steps_per_epoch)
        print(f"resumed {args.resume} at step {int(feed.cursor)} (epoch {first_epoch})")

    for ep in range(first_epoch, args.epochs):
        model.train()
        t1 = default_timer()
        train_l2 = torch.zeros((), device="cuda")  # noqa: F405
        if args.feed:
            for _ in range(feed.steps_per_epoch - (skip if ep == first_epoch else 0)):
                step.replay()                                         # the feed's launch is the first of the graph
                train_l2 += step.loss
        else:
            for x, y in loader:
                x, y = x.cuda(), y.cuda()
                if args.graph:
                    step.set_batch(x, y)
                    step.replay()
                    train_l2 += step.loss
                else:
                    optimizer.zero_grad()
                    out = model(mesh, x, mesh)
                    out = y_normalizer.denormalize(out)
                    loss = myloss(y, out)
                    loss.backward()
                    optimizer.step()
                    scheduler.step()
                    train_l2 += loss.detach()
        torch.cuda.synchronize()  # noqa: F405
        t2 = default_timer()
        model.eval()
        test = run_eval()
        t3 = default_timer()
        print(ep, f"{t2 - t1:.3f}s", float(train_l2) / args.ntrain, "| test", f"{t3 - t2:.3f}s", test.rel_lp / test.count,
              "worst sample", test.worst_rel_lp)
        if args.ema is not None:
            with opt.averaged():                                      # the same graph reads the average where the weights live
                avg = run_eval()
            print("   averaged weights (%d updates): test" % int(opt.n_averaged), avg.rel_lp / avg.count, "worst sample", avg.worst_rel_lp)
        if guarded:
            h = step.health(reset=True)                               # one read of the device state per epoch
            print(f"   guard: applied {h.applied} skipped {h.skipped} clipped {h.clipped} of {h.calls}; largest norm {h.max_norm:.4g}, "
                  f"last {h.norm:.4g} (coef {h.coef:.4g}); train loss per sample {h.mean_loss / args.batch:.6g} "
                  f"({h.nonfinite_loss} not finite)")
        if args.save is not None:
            torch.save(step.state_dict(), args.save.format(epoch=ep))  # noqa: F405
    torch.save({"model_state": model.state_dict()}, "/tmp/model.pth")  # noqa: F405


if __name__ == "__main__":
    main()
