"""The fused decoder's slabs as 4 x 4 patches of a row-major output grid (pit_slab_plan; csrc/pit_edge.hip): the grid
detector (CPU), the patch plan against a NumPy union of the oracle's keep-sets, and the decoder launches - forward, loss and every
gradient - against the oracle on the smallest grids where the slab -> row mapping can go wrong: partial patches on both edges
(9 x 9: a corner patch of one row; 10 x 7: width != height), no partial patch (12 x 12), the 16-slot tile on partial patches
(14 x 13), unions beyond 16 keys (the 32-slot tile on a patch plan), one and two heads, and the meshes that must keep consecutive slabs (a perturbed grid, a 1-D mesh, the switch).

The latent mesh is the smallest on which the fused decoder exists at all: a masked layer has candidate lists - and with them a
slab plan - only when three list capacities (32 entries at these localities) fit the row, n_in >= 96 (MeshPlan.__init__), so
the grids go against a 10 x 10 latent grid (the 1-D mesh against 96 points), not a 4 x 4 one.  Largest keepable union of a patch,
computed on the CPU: 9 x 9 24, 10 x 7 28, 12 x 12 16 and 14 x 13 14 (the 16-slot tile) at locality 0.02; 12 x 12 32 at locality 0.06."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_io as gio
import pit_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def grid(gw, gh):
    """(gw*gh, 2) row-major grid, coordinate 0 fastest: the point order of np.meshgrid(xs, ys) flattened (oracle grid_mesh_2d)."""
    xs, ys = np.linspace(0, 1, gw), np.linspace(0, 1, gh)
    return torch.tensor(np.vstack([a.ravel() for a in np.meshgrid(xs, ys)]).T, dtype=torch.float)


def perturbed(gw, gh):
    m = grid(gw, gh)
    m[3 * gw + 2, 0] += 1e-3
    return m


def keep_sets(mo, mi, loc, keepable=False):
    """(n_out, n_in) bool: the keys each row keeps at head scale 1 (pit.py:50: distance <= its row quantile).
    ``keepable``: the keys SOME head scale can keep - what a static plan must hold.  The mask compares fl(c m) with
    lerp(fl(c m_(k)), fl(c m_(k+1)), w) in fp32, so a key whose distance is within rounding of the threshold (on a grid: a key
    that ties with m_(k+1) in exact arithmetic and differs from it by an ulp in fp32) is kept at one c and not at another.  Every
    rounding of the decision (three products, the lerp's difference and fma, the lerp formed here) is below 2^-24 m_(k+1), nine
    of them in all: the plan's bound is lerp(m_(k), m_(k+1), w) + 2^-20 m_(k+1), the same fp32 expression as here - among the
    keys of the candidate lists the plan is built from, m <= m_(k+1) (1 + 2^-21) (include/pit_hip.h, pit_neighbors_fwd)."""
    d = orc.sqdist("euclid", mo, mi)
    if not keepable:
        return d <= orc.quantile_threshold(d, loc)
    mk, mk1, _ = orc.row_order_stats(d, loc)
    _, w = orc.quantile_rank(loc, mi.shape[0])
    listed = d <= (mk1 * torch.tensor(1.0 + 2.0 ** -21)).unsqueeze(-1)
    return listed & (d <= (orc.lerp_threshold(mk, mk1, w) + mk1 * torch.tensor(2.0 ** -20)).unsqueeze(-1))


def patch_rows(gw, gh, s, pw=4, ph=4):
    """mesh rows of patch s in slab-relative order (None: beyond the grid's edge)."""
    ppr = -(-gw // pw)
    pi, pj = divmod(s, ppr)
    out = []
    for r in range(pw * ph):
        i, j = pi * ph + r // pw, pj * pw + r % pw
        out.append(i * gw + j if (i < gh and j < gw) else None)
    return out


def patch_unions(mo, mi, loc, gw, gh, keepable=True):
    keep = keep_sets(mo, mi, loc, keepable).numpy()
    n_slabs = -(-gh // 4) * -(-gw // 4)
    return [np.flatnonzero(keep[[r for r in patch_rows(gw, gh, s) if r is not None]].any(0)).tolist() for s in range(n_slabs)]


# ------------------------------------------------------------------------------------------------ the grid detector (CPU)
def test_grid_detector_accepts_row_major_grids_only():
    from position_induced_transformer_amd import ops
    assert ops.row_major_grid(grid(9, 9)) == (9, 9)
    assert ops.row_major_grid(grid(10, 7)) == (10, 7)
    assert ops.row_major_grid(orc.grid_mesh_2d(43)) == (43, 43)
    assert ops.row_major_grid(orc.grid_mesh_2d(16, endpoint=False)) == (16, 16)
    xs, ys = np.linspace(0, 1, 10), np.linspace(0, 1, 7)
    col_major = torch.tensor(np.vstack([a.ravel() for a in np.meshgrid(xs, ys, indexing="ij")]).T, dtype=torch.float)
    assert ops.row_major_grid(col_major) is None                         # coordinate 1 fastest: np.meshgrid(..., indexing="ij")
    assert ops.row_major_grid(grid(10, 7).reshape(7, 10, 2).transpose(0, 1).reshape(-1, 2)) is None      # the same points, transposed
    assert ops.row_major_grid(perturbed(9, 9)) is None
    assert ops.row_major_grid(torch.linspace(0, 1, 65)[:-1].reshape(-1, 1)) is None                         # 1-D mesh
    assert ops.row_major_grid(grid(3, 12)) is None and ops.row_major_grid(grid(12, 3)) is None             # thinner than a patch
    assert ops.row_major_grid(torch.rand(81, 2, generator=torch.Generator().manual_seed(1))) is None
    assert ops.row_major_grid(grid(9, 9)[torch.randperm(81, generator=torch.Generator().manual_seed(2))]) is None


# ------------------------------------------------------------------------------------------------ the plan
@gpu
@pytest.mark.parametrize("gw,gh,lat,loc", [(9, 9, 10, 0.02), (10, 7, 10, 0.02), (12, 12, 10, 0.06)])
def test_patch_plan_holds_the_union_of_the_keep_sets_of_every_patch(gw, gh, lat, loc):
    """keys / nkeys of a patch plan = the sorted NumPy union, over the patch's valid rows, of the keys the oracle's mask can keep
    (keep_sets(keepable=True): its keep-set, and the keys within fp32 rounding of its threshold, which are kept or not depending
    on the head scale); that union contains the oracle's keep-set at scale 1 and exceeds it by near-ties only.  m and slot stay
    slab-relative: the row's distances in list order, every keepable candidate's slot pointing at its key, zero for rows beyond
    the grid's edge."""
    from position_induced_transformer_amd import ops
    mo, mi = grid(gw, gh), orc.grid_mesh_2d(lat)
    plan = ops.MeshPlan("euclid", mo.cuda(), mi.cuda(), loc, False)
    sp, max_union, (m, slot, keys, nkeys), _mc = plan.slab_plan(patch=True)
    assert (sp.grid_w, sp.grid_h, sp.patch_w, sp.patch_h) == (gw, gh, 4, 4)
    assert sp.n_slabs == -(-gh // 4) * -(-gw // 4) == keys.shape[0]
    unions = patch_unions(mo, mi, loc, gw, gh)
    assert nkeys.cpu().tolist() == [len(u) for u in unions]
    assert max_union == max(len(u) for u in unions)
    strict = patch_unions(mo, mi, loc, gw, gh, keepable=False)
    d = orc.sqdist("euclid", mo, mi)
    thr = orc.quantile_threshold(d, loc)
    for s, (u, v) in enumerate(zip(unions, strict)):
        assert set(v) <= set(u)
        rows = [r for r in patch_rows(gw, gh, s) if r is not None]
        for j in set(u) - set(v):                                        # an extra key ties with some row's threshold to 1e-6
            assert min(abs(float(d[r, j] / thr[r, 0]) - 1.0) for r in rows) <= 2e-6
    keep = keep_sets(mo, mi, loc, keepable=True)
    ref_m = ((mo[:, None, :] - mi[None, :, :]) ** 2).sum(-1)
    cap = plan.nbr_cap
    idx, cnt = plan.nbr_idx.view(plan.n_out, cap).cpu().long(), plan.nbr_cnt.cpu().long()
    m, slot, keys = m.cpu(), slot.cpu().long() & 0xffff, keys.cpu().long()
    for s, u in enumerate(unions):
        assert keys[s, :len(u)].tolist() == u
        for r, n in enumerate(patch_rows(gw, gh, s)):
            if n is None:
                assert not m[16 * s + r].any()
                continue
            c = int(cnt[n])
            assert torch.equal(m[16 * s + r, :c], ref_m[n, idx[n, :c]])
            for i in range(c):
                j = int(idx[n, i])
                if keep[n, j]:
                    assert int(keys[s, slot[16 * s + r, i]]) == j
    # the consecutive plan of the same pair is cached beside it, untouched
    assert plan.slab_plan()[0].patch_w == 0 and plan.slab_plan()[0].n_slabs == -(-gw * gh // 16)


# ------------------------------------------------------------------------------------------------ the decoder launches
def _decoder_case(mo, ltt, batch, heads, loc, seed):
    """pit.decoder through ops.decoder_apply against the oracle (tolerances of tests/test_gpu_round5.py: prediction 1e-5, d(values)
    and weight gradients 2e-5, d(lmda) 2e-4); returns the plan the launches ran on."""
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd import pit as P
    sdim = mo.shape[1]
    torch.manual_seed(seed)
    model = P.pit_fixed(sdim, 1, 1, 64, heads, 1, ltt.cuda(), loc, loc).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, ltt.shape[0], 64, generator=g)
    d_out = torch.randn(batch, mo.shape[0], 1, generator=g)
    xg, mog = x.cuda().requires_grad_(True), mo.cuda()
    calls = {"n": 0}
    orig = ops.decoder_apply

    def counting(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    ops.decoder_apply = counting
    try:
        with ops.head_scale_route("host"):
            out = model.decoder(model.mesh_ltt, xg, mog)
            out.backward(d_out.cuda())
    finally:
        ops.decoder_apply = orig
    torch.cuda.synchronize()
    assert calls["n"] == 1, "the fused decoder launch did not run"
    de = model.de
    xr, lm, w1, b1, w2, b2 = (t.detach().cpu().clone().requires_grad_(True)
                              for t in (x, model.up.lmda, de.mlp1.weight, de.mlp1.bias, de.mlp2.weight, de.mlp2.bias))
    ref = orc.mlp(orc.posatt_cross("euclid", False, mo, ltt, xr, lm, loc), w1, b1, w2, b2)
    ref.backward(d_out)
    assert gio.rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-5
    assert gio.rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) <= 2e-5, "d(values)"
    for name, a, r in (("w1", de.mlp1.weight, w1), ("b1", de.mlp1.bias, b1), ("w2", de.mlp2.weight, w2), ("b2", de.mlp2.bias, b2)):
        assert gio.rel_l2(a.grad.cpu().numpy(), r.grad.numpy()) <= 2e-5, name
    assert float((model.up.lmda.grad.cpu().reshape(-1) - lm.grad.reshape(-1)).norm()) <= 2e-4 * float(lm.grad.norm()), "d(lmda)"
    return model.up._plan(mog, model.mesh_ltt, False)


GRID_CASES = [  # gw, gh, latent side, batch, heads, locality
    (9, 9, 10, 4, 2, 0.02), (9, 9, 10, 4, 1, 0.02), (10, 7, 10, 4, 2, 0.02), (12, 12, 10, 2, 2, 0.02), (12, 12, 10, 2, 1, 0.02),
    (12, 12, 10, 2, 2, 0.06), (12, 12, 10, 2, 1, 0.06), (14, 13, 10, 2, 2, 0.02), (14, 13, 10, 2, 1, 0.02),
]


@gpu
@pytest.mark.parametrize("gw,gh,lat,batch,heads,loc", GRID_CASES)
def test_fused_decoder_on_patch_slabs_against_the_oracle(gw, gh, lat, batch, heads, loc):
    mo, ltt = grid(gw, gh), orc.grid_mesh_2d(lat)
    plan = _decoder_case(mo, ltt, batch, heads, loc, 61)
    sp, max_union = plan.slab_plan(patch=True)[:2]
    assert (sp.grid_w, sp.grid_h, sp.patch_w, sp.patch_h) == (gw, gh, 4, 4), "the decoder did not run on a patch plan"
    assert sp.n_slabs == -(-gh // 4) * -(-gw // 4)
    largest = max(len(u) for u in patch_unions(mo, ltt, loc, gw, gh))
    assert max_union == largest
    # 12 x 12 and 14 x 13 (partial patches on both edges) at locality 0.02: the 16-slot tile; every other case: unions of 17 to 32
    # keys - the 32-slot instance on a patch plan
    assert (largest <= 16) if (gw, loc) in ((12, 0.02), (14, 0.02)) else (16 < largest <= 32)
    if (gw, gh) == (12, 12):
        assert sp.n_slabs == plan.slab_plan()[0].n_slabs == 9            # no partial patch: as many slabs as consecutive ones


@gpu
def test_perturbed_grid_keeps_consecutive_slabs():
    plan = _decoder_case(perturbed(9, 9), orc.grid_mesh_2d(10), 4, 2, 0.02, 63)
    sp = plan.slab_plan(patch=True)[0]
    assert sp.patch_w == 0 and sp.n_slabs == 6 and plan._patch is False


@gpu
def test_one_dimensional_mesh_keeps_consecutive_slabs():
    mo, ltt = torch.linspace(0, 1, 65)[:-1].reshape(-1, 1), torch.linspace(0, 1, 97)[:-1].reshape(-1, 1)
    plan = _decoder_case(mo, ltt, 4, 2, 0.05, 65)
    sp = plan.slab_plan(patch=True)[0]
    assert sp.patch_w == 0 and sp.n_slabs == 4 and plan._patch is False


@gpu
def test_switch_gives_consecutive_slabs_and_the_same_results():
    """PIT_PATCH_SLABS=0 (read once per process: a child) runs the 9 x 9 case on consecutive slabs within the same tolerances."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import pit_oracle as orc, test_gpu_patch_slabs as t\n"
            "from position_induced_transformer_amd import ops\n"
            "assert not ops.PATCH_SLABS\n"
            "plan = t._decoder_case(t.grid(9, 9), orc.grid_mesh_2d(10), 4, 2, 0.02, 61)\n"
            "sp = plan.slab_plan(patch=True)[0]\n"
            "assert sp.patch_w == 0 and sp.n_slabs == 6 and plan._patch is None\n"
            "print('consecutive ok')\n") % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PIT_PATCH_SLABS="0"), capture_output=True, text=True,
                         cwd=ROOT, timeout=300)
    assert res.returncode == 0 and "consecutive ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ the loss inside the launches
@gpu
@pytest.mark.parametrize("gw,gh,batch,affine", [(9, 9, 4, True), (10, 7, 4, False)])
def test_train_step_with_the_loss_on_patch_slabs_matches_the_oracle(gw, gh, batch, affine):
    """engine.TrainStep: the RelL2 loss is accumulated per PATCH by the decoder's forward launch (one fp64 pair per slab of the
    plan) and differentiated by its backward launch; prediction, loss and every gradient against the oracle's step."""
    from position_induced_transformer_amd import ops, tasks
    from position_induced_transformer_amd.engine import TrainStep
    mesh, ltt = grid(gw, gh), orc.grid_mesh_2d(10)
    torch.manual_seed(71)
    model = tasks.pit_darcy(2, 1, 1, 64, 2, 1, ltt.cuda(), 0.02, 0.02).cuda()
    g = torch.Generator().manual_seed(72)
    mesh_g = mesh.reshape(gh, gw, 2).cuda()
    b4 = (mesh_g, torch.randn(batch, gh, gw, 1, generator=g).cuda(), mesh_g, torch.randn(batch, gh, gw, 1, generator=g).cuda())
    aff = (torch.rand(gh, gw, 1, generator=g).cuda() + 0.5, torch.randn(gh, gw, 1, generator=g).cuda()) if affine else None
    fused = {"n": 0, "dec": 0}
    orig_loss, orig_dec = ops._FusedLoss.apply, ops.decoder_apply

    def counting_loss(*a, **k):
        fused["n"] += 1
        return orig_loss(*a, **k)

    def counting_dec(*a, **k):
        fused["dec"] += 1
        return orig_dec(*a, **k)
    ops._FusedLoss.apply, ops.decoder_apply = counting_loss, counting_dec
    try:
        with ops.head_scale_route("host"):
            step = TrainStep(model, b4, 1, 2, pred_affine=aff)
            step.run_eager()
            step.run_eager()
    finally:
        ops._FusedLoss.apply, ops.decoder_apply = orig_loss, orig_dec
    torch.cuda.synchronize()
    assert fused["dec"] >= 1 and fused["n"] >= 1, "the fused decoder / the loss inside it did not run"
    plan = model.up._plan(mesh_g.reshape(-1, 2), model.mesh_ltt, False)
    sp = plan.slab_plan(patch=True)[0]
    assert sp.patch_w == 4 and sp.n_slabs == -(-gh // 4) * -(-gw // 4)
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    f = orc.with_coords(mesh, b4[1].cpu().reshape(batch, -1, 1))
    ref = orc.pit_apply(sd, "euclid", False, 1, 0.02, 0.02, mesh, f, ltt, mesh).reshape(b4[3].shape)
    pred = ref if aff is None else ref * aff[0].cpu() + aff[1].cpu()
    ref_loss = orc.rel_lp_loss(b4[3].cpu(), pred, 1, 2)
    ref_loss.backward()
    assert gio.rel_l2(step.out.cpu().numpy(), ref.detach().numpy()) <= 1e-5
    assert abs(float(step.loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    lk = [k for k in sd if k.endswith("lmda")]
    for k, q in model.named_parameters():
        if not k.endswith("lmda"):
            assert gio.rel_l2(q.grad.cpu().numpy(), sd[k].grad.numpy()) <= 2e-5, k
    got = torch.cat([dict(model.named_parameters())[k].grad.cpu().reshape(-1) for k in lk])
    want = torch.cat([sd[k].grad.reshape(-1) for k in lk])
    assert float((got - want).norm()) <= 2e-4 * float(want.norm()), "d(lmda)"
