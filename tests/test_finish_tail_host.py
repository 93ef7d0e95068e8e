"""Host side of the finishing launch's staged jobs (no GPU): the header's addition, the schedule function that decides which
launch of a fused processor's backward carries which weight-gradient job (ops.rider_tail_schedule), and the table the
postponed jobs wait in (ops._PENDING_TAIL): every job of a pass is performed exactly once, whichever callback runs first."""
import itertools
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pit_hip.h")


def test_header_and_binding_declare_the_addition():
    from position_induced_transformer_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^#define PIT_HAS_FINISH_TAIL 1$", text, flags=re.M)
    assert _lib.DEFINES["PIT_HAS_FINISH_TAIL"] == 1 and _lib.ABI_VERSION == 31
    for name in ("pit_posatt_dhead_finish_stage", "pit_finish_last_tail"):
        assert name in _lib.ADDED_LATER and name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, text), name
    assert len(_lib.SIGNATURES["pit_posatt_dhead_finish_stage"]) == 2
    slots = {n: int(v) for n, v in re.findall(r"#define PIT_FINISH_TAIL_(\w+)\s+(\d+)\b", text)}
    assert slots.pop("SLOTS") == len(slots) == 6 and sorted(slots.values()) == list(range(6))
    assert _lib.DEFINES["PIT_RIDER_KINDS"] == 9           # the counter kinds stay
    # the finish entry keeps its signature: nine arguments, the rider last but one
    assert _lib.PROTOTYPES["pit_posatt_dhead_finish"].argnames[-2:] == ["rider", "stream"]
    assert len(_lib.SIGNATURES["pit_posatt_dhead_finish"]) == 9


def _jobs_of(n, n_slices, plan):
    """Every (job, destination) of a pass under `plan`: the n own jobs and the slices."""
    out = []
    for j, (own, sl) in enumerate(plan):
        out.append((("own", j), own if own == "tail" else ("launch", j)))
        if sl is not None:
            out.append((("slice", j), sl if sl == "tail" else ("launch", j)))
    return out


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_schedule_clamps_k_and_places_every_job_once(n):
    from position_induced_transformer_amd.ops import rider_tail_schedule
    for k in (-3, 0, 1, 2, n, n + 1, 99):
        k_eff, n_slices, plan = rider_tail_schedule(n, k)
        assert k_eff == max(0, min(k, n)) and n_slices == n and len(plan) == n
        jobs = _jobs_of(n, n_slices, plan)
        assert sorted(j for j, _ in jobs) == sorted([("own", j) for j in range(n)] + [("slice", j) for j in range(n)])
        for (kind, j), dest in jobs:                       # the last k_eff launches carry nothing, the others what they always did
            assert dest == ("tail" if j >= n - k_eff else ("launch", j)), (n, k, kind, j, dest)
    # no postponed decoder job: own jobs only
    k_eff, n_slices, plan = rider_tail_schedule(n, 1, has_slices=False)
    assert k_eff == 1 and n_slices == 0 and all(sl is None for _, sl in plan)
    assert [own for own, _ in plan] == ["launch"] * (n - 1) + ["tail"]


@pytest.mark.parametrize("n,complete_by", [(4, 2), (4, 0), (5, 4), (2, 1)])
def test_schedule_under_a_two_bucket_hook_keeps_every_slice_early(n, complete_by):
    from position_induced_transformer_amd.ops import rider_tail_schedule
    for k in (0, 1, n):
        k_eff, n_slices, plan = rider_tail_schedule(n, k, complete_by=complete_by)
        assert k_eff == 0 and n_slices == max(1, n - complete_by)
        assert all(own == "launch" for own, _ in plan)
        # slice j rides in launch j = block n - 1 - j >= complete_by
        assert [sl for _, sl in plan] == ["launch"] * n_slices + [None] * (n - n_slices)
        assert all(n - 1 - j >= complete_by for j, (_, sl) in enumerate(plan) if sl is not None) or n_slices == 1


def test_schedule_forces_k_to_zero_where_jobs_cannot_wait():
    from position_induced_transformer_amd.ops import rider_tail_schedule
    flags = ("reproducible", "inplace", "heads_deferred", "chain_fits")
    for values in itertools.product([False, True], repeat=4):
        kw = dict(zip(flags, values))
        k_eff, _, plan = rider_tail_schedule(4, 2, **kw)
        want = 2 if (not kw["reproducible"] and kw["inplace"] and kw["heads_deferred"] and kw["chain_fits"]) else 0
        assert k_eff == want, kw
        assert sum(own == "tail" for own, _ in plan) == want


class _Stream:
    def __init__(self, index):
        self.device = type("D", (), {"index": index})()


def test_tail_table_runs_every_job_once_whichever_callback_is_first(monkeypatch):
    """_tail_take (the finishing launch's side) and _tail_end_of_pass (the callback) on fake jobs: a pass without a finishing
    launch performs the tail jobs itself; what the finishing launch took is not run again."""
    import torch
    from position_induced_transformer_amd import ops
    ran, queued = [], []
    s0, s1 = _Stream(0), _Stream(0)
    monkeypatch.setattr(ops, "_dw_run", lambda job: ran.append(job[0]))
    monkeypatch.setattr(ops, "_graph_task", lambda: 7)
    monkeypatch.setattr(ops, "_at_end_of_pass", lambda fn: queued.append(fn))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: s0)
    monkeypatch.setattr(ops, "_PENDING_TAIL", {})
    # a pass that ends without a finishing launch
    ops._tail_defer([("a", (), s0)])
    ops._tail_defer([("b", (), s0), ("c", (), s1)])
    assert len(queued) == 1, "one end-of-pass callback per pass"
    ops._flush_head_finishes(7)                            # (no deferred d(lmda): no launch, the table is not touched)
    assert ran == [] and len(ops._PENDING_TAIL[7]) == 3
    queued.pop()()
    assert ran == ["a", "b", "c"] and 7 not in ops._PENDING_TAIL
    ops._tail_end_of_pass(7)
    assert ran == ["a", "b", "c"]
    # the finishing launch first: it takes the jobs of its device and stream, the callback the rest
    ran.clear()
    ops._tail_defer([("a", (), s0), ("c", (), s1), ("b", (), s0)])
    assert [j[0] for j in ops._tail_take(7, 0)] == ["a", "b"]
    assert ops._tail_take(7, 0) == [] and ops._tail_take(7, 1) == []
    queued.pop()()
    assert ran == ["c"] and 7 not in ops._PENDING_TAIL


def test_switch_is_an_integer_attribute_read_once():
    from position_induced_transformer_amd import ops
    assert isinstance(ops.RIDER_TAIL_BLOCKS, int) and ops.RIDER_TAIL_BLOCKS >= 0
