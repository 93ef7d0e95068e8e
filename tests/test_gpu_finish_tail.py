"""The finishing launch carrying staged weight-gradient jobs (pit_posatt_dhead_finish_stage -> pit_posatt_dhead_finish ->
posatt_dhead_finish_tail) and the placement that feeds it (ops.RIDER_TAIL_BLOCKS).

1. Raw ABI: one layer (H = 2, accumulators pre-filled), `rider` none or an encoder-shaped job, staged jobs of the shapes the
   processor's last launches give up.  Every job against fp64 of its own buffers (test_gpu_riders._check_job: rel-L2 2e-6 and
   (K + 2) u elementwise, bounds that hold for any summation order), its inputs unchanged, the canaries around its gradient
   slots intact; d_head bit-equal with and without staged jobs; pit_finish_last_tail and pit_debug_rider_counts tell what
   was carried and what ran on its own.
2. A whole pass at the smallest shape the fused processor takes (16 x 16 latent grid, hid 64, 2 heads, 2 blocks, batch 2, a
   12 x 12 grid either side), k = 0, 1, 2: gradients against the k = 0 pass, the last block launch without riders, the record,
   and the same step captured and replayed (a staged pointer that outlived its struct shows there).
"""
import ctypes

import pytest
import torch

import golden_io as gio
from test_gpu_fused_envelope import lattice
from test_gpu_riders import KINDS, Job, _counts

pytestmark = pytest.mark.gpu

SLOTS = ("staged", "carried", "rd", "tile", "thin", "own")       # PIT_FINISH_TAIL_*
STAGED_MAX = 8                                                   # staged jobs one finishing launch carries
H = 2


def _record():
    from position_induced_transformer_amd import _lib
    out = (ctypes.c_int * len(SLOTS))()
    assert _lib.lib().pit_finish_last_tail(out, len(SLOTS)) == len(SLOTS) == _lib.DEFINES["PIT_FINISH_TAIL_SLOTS"]
    return dict(zip(SLOTS, out))


def _finish(staged=(), rider=None, n_layers=1, seed=7):
    """Stage `staged` (Job objects), then one finish call of `n_layers` layers with `rider`: (d_head, the record, the rider counts
    noted by the staging call, those noted by the finish call)."""
    from position_induced_transformer_amd import _lib
    g = torch.Generator().manual_seed(seed)
    head = torch.rand(H, generator=g).cuda() + 0.5
    ws = (torch.randn(H * 1024, generator=g, dtype=torch.float64) * 1e-3).cuda()
    dh = torch.zeros(H, device="cuda")
    L = _lib.lib()
    _counts()
    if staged:
        arr = (ctypes.c_void_p * len(staged))(*[ctypes.addressof(j.st) for j in staged])
        _lib.check(L.pit_posatt_dhead_finish_stage(arr, len(staged)), "pit_posatt_dhead_finish_stage")
        del arr                                         # (the entry copies: nothing of the caller's is read later)
    noted_stage = _counts()
    one = lambda t, *v: (t * max(1, n_layers))(*v)      # noqa: E731
    rc = L.pit_posatt_dhead_finish(n_layers, one(ctypes.c_void_p, ws.data_ptr()), one(ctypes.c_void_p, dh.data_ptr()),
                                   one(ctypes.c_void_p, head.data_ptr()), one(ctypes.c_void_p, None), one(ctypes.c_int, H),
                                   one(ctypes.c_int, 0), rider.ptr if rider is not None else None, _lib.stream_ptr())
    _lib.check(rc, "pit_posatt_dhead_finish")
    noted_finish = _counts()
    torch.cuda.synchronize()
    if n_layers:
        assert float(ws.abs().max()) == 0.0, "workspace not drained"
    return dh, _record(), noted_stage, noted_finish


def _block_job(rows, seed):
    return Job(rows, 192, 64, 64, 1, 192, 64, 0, seed)             # a block's own MLP: (1 + H) 64 -> 64 -> 64, trailing gelu


def _thin_job(rows, ld_dy, seed):
    return Job(rows, 128, 64, 1, 0, 128, ld_dy, 0, seed)           # a decoder slice: 128 -> 64 -> 1, no trailing gelu


def _encoder_job(seed):
    return Job(256, 6, 64, 64, 1, 8, 64, 0, seed)                  # 6 -> 64 -> 64 on 256 rows


ZERO = dict.fromkeys(SLOTS, 0)


def test_finish_without_staged_jobs_leaves_the_record_at_zero():
    """After a call that carried a staged job, a call with nothing staged: the record is all zero again, d_head the same bits,
    and the rider is noted as ever."""
    dh1, rec1, _, _ = _finish([_block_job(256, 11)])
    assert rec1["staged"] == 1 and rec1["carried"] == 1
    rider = _encoder_job(12)
    dh0, rec0, noted_stage, noted_finish = _finish(rider=rider)
    assert rec0 == ZERO and noted_stage == {} and noted_finish == {"dhead_finish": 1}
    rider.check(False, "rider, nothing staged")
    assert torch.equal(dh0.view(torch.int32), dh1.view(torch.int32))
    assert set(KINDS) >= set(noted_finish)


@pytest.mark.parametrize("with_rider", [False, True], ids=["no-rider", "encoder-rider"])
@pytest.mark.parametrize("rows", [256, 259])
def test_block_shaped_job_rides_as_tiles(rows, with_rider):
    """192 -> 64 -> 64 with trailing gelu, 256 rows (four whole chunks) and 259 (a masked last chunk): 1 + 3 tiles on two slabs."""
    plain, _, _, _ = _finish()
    job, rider = _block_job(rows, 21), (_encoder_job(22) if with_rider else None)
    dh, rec, noted_stage, noted_finish = _finish([job], rider)
    assert rec == dict(ZERO, staged=1, carried=1, tile=8), rec
    assert noted_stage == {"dhead_finish": 1} and noted_finish == ({"dhead_finish": 1} if with_rider else {})
    job.check(True, f"block job, {rows} rows")
    if rider is not None:
        rider.check(False, "rider beside a staged job")
    assert torch.equal(dh.view(torch.int32), plain.view(torch.int32)), "d_head depends on the staged jobs"


@pytest.mark.parametrize("ld_dy", [1, 4])
@pytest.mark.parametrize("rows", [1, 17, 259, 3698])
def test_thin_job_rides_as_a_row_reduction(rows, ld_dy):
    """128 -> 64 -> 1 without trailing gelu: dW2 | db2 on max(1, min(16, rows // 128)) thin workgroups, dW1 | db1 beside it."""
    plain, _, _, _ = _finish()
    job = _thin_job(rows, ld_dy, 31)
    dh, rec, noted_stage, noted_finish = _finish([job])
    assert (rec["staged"], rec["carried"], rec["own"]) == (1, 1, 0), rec
    assert rec["thin"] == max(1, min(16, rows // 128)) and rec["tile"] + rec["rd"] > 0, rec
    assert noted_stage == {"dhead_finish": 1} and noted_finish == {}
    job.check(True, f"thin job, {rows} rows, ld_dy {ld_dy}")
    assert torch.equal(dh.view(torch.int32), plain.view(torch.int32))


@pytest.mark.parametrize("extra", [0, 1], ids=["N", "N+1"])
def test_as_many_jobs_as_the_launch_holds_and_one_more(extra):
    """N staged jobs all ride; of N + 1 the last runs as a launch of its own, noted as such by the staging call."""
    jobs = [_block_job(64 + 3 * i, 40 + i) for i in range(STAGED_MAX + extra)]
    rider = _encoder_job(39)
    _, rec, noted_stage, noted_finish = _finish(jobs, rider)
    assert (rec["staged"], rec["carried"], rec["own"]) == (STAGED_MAX + extra, STAGED_MAX, extra), rec
    assert noted_stage == dict({"dhead_finish": STAGED_MAX}, **({"own": 1} if extra else {}))
    assert noted_finish == {"dhead_finish": 1}
    for i, j in enumerate(jobs):
        j.check(i < STAGED_MAX, f"job {i} of {len(jobs)}")
    rider.check(False, "rider beside N staged jobs")


def test_job_that_does_not_accumulate_runs_on_its_own():
    a, b = _block_job(256, 51), _thin_job(259, 4, 52)
    a.st.accumulate = 0
    _, rec, noted_stage, noted_finish = _finish([a, b])
    assert (rec["staged"], rec["carried"], rec["own"]) == (2, 1, 1), rec
    assert noted_stage == {"dhead_finish": 1, "own": 1} and noted_finish == {}
    a.check(False, "accumulate = 0")
    b.check(True, "beside a job that fell back")


def test_staged_jobs_without_layers_run_on_their_own():
    """n_layers = 0: no finishing launch - the rider and every staged job as launches of their own, none lost, none twice."""
    a, b, rider = _block_job(259, 61), _thin_job(17, 1, 62), _encoder_job(63)
    _, rec, _, noted_finish = _finish([a, b], rider, n_layers=0)
    assert (rec["staged"], rec["carried"], rec["own"]) == (2, 0, 2), rec
    assert noted_finish == {"own": 1}                   # (the rider's; staged jobs are noted by the staging call alone)
    for j, what in ((a, "block job"), (b, "thin job"), (rider, "rider")):
        j.check(False, what + ", n_layers = 0")


def test_launch_beyond_two_workgroups_per_compute_unit_takes_more_rows_per_tile():
    """Two jobs of 8 192 rows of the block shape are 2 x 4 tiles x 64 slabs at two chunks per tile, 512 workgroups beside the two
    that drain; with more chunks per tile for one of them the whole launch is resident at once (two 64 KiB workgroups per compute
    unit), and the sums are the same sums."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    jobs = [_block_job(8192, 71), _block_job(8192, 72)]
    _, rec, _, _ = _finish(jobs)
    assert rec["carried"] == 2 and rec["own"] == 0 and 0 < rec["tile"] < 512, rec
    if cus >= 64:
        assert H + rec["tile"] <= 2 * cus, (rec, cus)
    for j in jobs:
        j.check(True, "8192 rows, beyond the resident set")


# --------------------------------------------------------------------------- 2. a whole pass
def _step_setup(seed=81):
    from position_induced_transformer_amd import tasks
    mesh, ltt = lattice((12, 12), seed), lattice((16, 16), seed + 1)
    torch.manual_seed(seed + 2)
    model = tasks.pit_darcy(2, 1, 1, 64, H, 2, ltt.cuda(), 0.02, 0.02).cuda()
    g = torch.Generator().manual_seed(seed + 3)
    mesh_g = mesh.reshape(12, 12, 2).cuda()
    b4 = (mesh_g, torch.randn(2, 12, 12, 1, generator=g).cuda(), mesh_g, torch.randn(2, 12, 12, 1, generator=g).cuda())
    return model, b4


class _BlockLog:
    """(rider given, rider2 given) of every pit_block_bwd call, in call order."""

    def __enter__(self):
        from position_induced_transformer_amd import _lib
        self.L, self.real, self.calls = _lib.lib(), _lib.lib().pit_block_bwd, []

        def spy(*a):
            self.calls.append((a[-4] is not None, a[-3] is not None))
            return self.real(*a)
        self.L.pit_block_bwd = spy
        return self

    def __exit__(self, *exc):
        self.L.pit_block_bwd = self.real


def _grads(model):
    return {k: q.grad.detach().clone() for k, q in model.named_parameters()}


def _last_block_riders():
    from position_induced_transformer_amd import _lib
    out = (ctypes.c_int * 5)()
    assert _lib.lib().pit_block_bwd_last_riders(out, 5) == 5
    return tuple(out)


def _close(got, ref, again, what):
    for k in ref:
        a, b, c = (t.double().cpu().numpy().reshape(-1) for t in (ref[k], got[k], again[k]))
        noise = gio.rel_l2(c, a)
        err = gio.rel_l2(b, a)
        print(f"{what} {k}: {err:.3e} (two identical passes {noise:.3e})")
        assert err <= max(2e-6, 4 * noise), (what, k, err, noise)


@pytest.fixture(scope="module")
def eager_reference():
    """The k = 0 pass twice (the reference and its run-to-run distance) with the launch log of the first."""
    from position_induced_transformer_amd import ops, utils
    from position_induced_transformer_amd.ddp import FlatGradients
    model, b4 = _step_setup()
    loss_fn = utils.RelLpNorm(1, 2)
    flat = FlatGradients(model.parameters())
    saved = ops.RIDER_TAIL_BLOCKS

    def run(k):
        ops.RIDER_TAIL_BLOCKS = k
        try:
            flat.zero_()
            with _BlockLog() as log:
                loss_fn(b4[3], model(*b4[:3])).backward()
            torch.cuda.synchronize()
        finally:
            ops.RIDER_TAIL_BLOCKS = saved
        assert not ops._PENDING_TAIL, "tail jobs left after the pass"
        return _grads(model), log.calls, _record(), _last_block_riders()
    ref, calls0, rec0, _ = run(0)
    again = run(0)[0]
    assert rec0 == ZERO and len(calls0) == 2 and all(c[0] for c in calls0), (rec0, calls0)
    return model, b4, run, ref, again, calls0


@pytest.mark.parametrize("k", [0, 1, 2])
def test_whole_pass_with_the_last_k_launches_bare(k, eager_reference):
    model, b4, run, ref, again, calls0 = eager_reference
    got, calls, rec, last = run(k)
    _close(got, ref, again, f"k={k}")
    n = len(calls0)
    assert len(calls) == n
    for j in range(n):
        assert calls[j] == (calls0[j] if j < n - k else (False, False)), (k, j, calls, calls0)
    moved = sum(int(r) + int(r2) for r, r2 in calls0[n - k:]) if k else 0
    assert (rec["staged"], rec["carried"], rec["own"]) == (moved, moved, 0), (k, rec, calls0)
    if k >= 1:
        assert last == (0, 0, 0, 0, 0), last            # block 0's launch, the pass's last: nothing rides


@pytest.mark.parametrize("k", [1, 2])
def test_captured_step_replayed(k, eager_reference):
    """engine.TrainStep captured with the last k launches bare, replayed three times: the gradients of every replay against the
    eager TrainStep at k = 0."""
    from position_induced_transformer_amd import ops
    from position_induced_transformer_amd.engine import TrainStep
    model, b4, _run, _ref, _again, calls0 = eager_reference
    saved = ops.RIDER_TAIL_BLOCKS
    try:
        ops.RIDER_TAIL_BLOCKS = 0
        eager = TrainStep(model, b4, 1, 2)
        eager.run_eager()
        torch.cuda.synchronize()
        ref = _grads(model)
        eager.run_eager()
        torch.cuda.synchronize()
        again = _grads(model)
        ops.RIDER_TAIL_BLOCKS = k
        step = TrainStep(model, b4, 1, 2)
        step.capture()
        rec = _record()
        for r in range(3):
            step.replay()
            torch.cuda.synchronize()
            _close(_grads(model), ref, again, f"k={k} replay {r}")
    finally:
        ops.RIDER_TAIL_BLOCKS = saved
    moved = sum(int(r) + int(r2) for r, r2 in calls0[len(calls0) - k:])
    assert (rec["staged"], rec["carried"], rec["own"]) == (moved, moved, 0), (k, rec)
    assert not ops._PENDING_TAIL
