"""CPU: pit_debug_dense_counts (PIT_HAS_DENSE_COUNTS, an addition to ABI 31), the launch record of the dense position-attention
launchers of csrc/pit_posatt.hip.  What needs no device: the entry is in the header-derived binding, it reports the header's slot
count, copies min(n, kinds) slots, accepts out = NULL, its reset leaves zeros, and every thread reads a record of its own.  The
non-zero record - counters and last-launch slots per instance, the reset of a non-zero record, its thread locality next to real
launches - is asserted on the GPU (tests/test_gpu_dense_edges.py)."""
import ctypes
import os
import re
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_slots():
    header = open(os.path.join(ROOT, "include", "pit_hip.h")).read()
    assert re.search(r"#define PIT_HAS_DENSE_COUNTS 1", header)
    slots = {name: int(v) for name, v in re.findall(r"#define PIT_DENSE_(\w+)\s+(\d+)\b", header)}
    return slots, slots.pop("KINDS")


def test_dense_record_slots_match_the_header_and_the_binding():
    from position_induced_transformer_amd import _lib
    slots, kinds = _header_slots()
    assert sorted(slots.values()) == list(range(kinds))                    # one slot per name, none twice
    counters = [n for n in slots if not n.startswith("LAST_")]
    assert len(counters) == 11 and max(slots[n] for n in counters) < min(v for n, v in slots.items() if n.startswith("LAST_"))
    assert "pit_debug_dense_counts" in _lib.SIGNATURES and "pit_debug_dense_counts" in _lib.ADDED_LATER
    assert _lib.DEFINES["PIT_DENSE_KINDS"] == kinds and all(_lib.DEFINES["PIT_DENSE_" + n] == v for n, v in slots.items())
    assert _lib.lib().pit_debug_dense_counts(None, 0, 0) == kinds
    # the coarse counter and the size of the record that existing tests index stay where they were
    assert _lib.DEFINES["PIT_ATT_DENSE"] == 21 and _lib.DEFINES["PIT_ATT_KINDS"] == 28


def test_dense_record_copies_what_fits_resets_and_is_per_thread():
    from position_induced_transformer_amd import _lib, ops
    _, kinds = _header_slots()
    fn = _lib.lib().pit_debug_dense_counts
    assert fn(None, kinds, 1) == kinds                                     # reset with out = NULL
    for n in (0, 3, kinds, kinds + 5):
        buf = (ctypes.c_int * (kinds + 5))(*([-1] * (kinds + 5)))
        assert fn(buf, n, 0) == kinds
        assert list(buf) == [0] * min(n, kinds) + [-1] * (kinds + 5 - min(n, kinds))
    assert ops.dense_launch_counts() == [0] * kinds and ops.dense_launch_counts(reset=True) == [0] * kinds
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.dense_launch_counts(reset=True)))
    t.start()
    t.join()
    assert seen == [[0] * kinds]
    # the two records are separate objects: resetting one is not resetting the other's length or contents
    assert len(ops.att_launch_counts()) == _lib.DEFINES["PIT_ATT_KINDS"]
