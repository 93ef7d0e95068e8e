"""Argument refusals of the layer entries beside the main mesh path - the four pit_posatt_ragged* entries, pit_posatt_dmesh,
pit_distmat_fwd / _bwd and pit_distlist_fwd / _bwd - as a table: a valid call with ONE argument changed, and the code it gets.
Every row returns before any launch, so no GPU is needed (the pointers are host memory and are never dereferenced)."""
import ctypes

import pytest

NULL, SIZE, UNSUPPORTED = -1, -2, -4                                 # PIT_ERR_* of include/pit_hip.h
BIG = 1 << 30                                                        # rows this far apart: two of them exceed a buffer descriptor

_buf = (ctypes.c_float * 64)()
P = ctypes.addressof(_buf)

VALUES = dict(values=P, dim=2, ld_values=2, values_bstride=18)
HEAD = dict(head=P, n_head=1, head_is_scale=1)
OUT = dict(out=P, ld_out=2, out_bstride=8, out_col0=0, copy_inputs=0)
DOUT = dict(d_out=P, ld_dout=2, dout_bstride=8, out_col0=0)
DVALUES = dict(d_values=P, ld_dvalues=2, dvalues_bstride=18, add_residual=0)
DHEAD = dict(d_head=P, accumulate_head=0, workspace=P)
TAIL = dict(math_mode=0, stream=None)

RAGGED = dict(mesh_out=P, mesh_in=P, mesh_batch=2, n_out=4, n_in=9, space_dim=2, len_out=P, len_in=P)
RAGGED_STRIDED = dict(mesh_out=P, mesh_in=P, mesh_batch=2, n_out=4, n_in=9, space_dim=2, out_stride=4, in_stride=0, len_out=None, len_in=None)
RAGGED_FWD = dict(**VALUES, **HEAD, stats=P, rank_w=P, masked=1, **OUT, rowstat=P, scale_out=None,
                  nbr_idx=None, nbr_cnt=None, nbr_cap=0, **TAIL)
RAGGED_BWD = dict(**VALUES, **HEAD, scale=None, rowstat=P, masked=1, **DOUT, **DVALUES, **DHEAD,
                  nbr_idx=None, nbr_cnt=None, nbr_cap=0, rev_ptr=None, rev_row=None, **TAIL)
MAT = dict(m=P, ld_m=9, m_bstride=0, n_out=4, n_in=9)
LIST = dict(idx=P, sqd=P, ld=4, bstride=0, cap=4, n_out=4, n_in=9)
DIST_VALUES = dict(values=P, batch=2, dim=2, ld_values=2, values_bstride=18)
DIST_FWD = dict(**DIST_VALUES, **HEAD, stats=P, rank_w=0.5, masked=1, **OUT, rowstat=P, scale_out=None, **TAIL)
DIST_BWD = dict(**DIST_VALUES, **HEAD, scale=None, rowstat=P, masked=1, **DOUT, **DVALUES, **DHEAD)

ENTRIES = {
    "pit_posatt_ragged_fwd": dict(**RAGGED, **RAGGED_FWD),
    "pit_posatt_ragged_strided_fwd": dict(**RAGGED_STRIDED, **RAGGED_FWD),
    "pit_posatt_ragged_bwd": dict(**RAGGED, **RAGGED_BWD),
    "pit_posatt_ragged_strided_bwd": dict(**RAGGED_STRIDED, **RAGGED_BWD),
    "pit_posatt_dmesh": dict(mesh_out=P, mesh_in=P, mesh_batch=2, n_out=4, n_in=9, space_dim=2, metric=0, period=0.0,
                             **DIST_VALUES, **HEAD, scale=None, rowstat=P, masked=1, **DOUT,
                             nbr_idx=None, nbr_cnt=None, nbr_cap=0, nbr_complete=0, rev_ptr=None, rev_row=None,
                             d_mesh_out=P, d_mesh_in=P, accumulate=0, workspace=P, stream=None),
    "pit_distmat_fwd": dict(**MAT, **DIST_FWD),
    "pit_distmat_bwd": dict(**MAT, **DIST_BWD, d_m=P, out=P, ld_out=2, out_bstride=8, a_workspace=P, **TAIL),
    "pit_distlist_fwd": dict(**LIST, **DIST_FWD),
    "pit_distlist_bwd": dict(**LIST, **DIST_BWD, d_sqd=P, out=P, ld_out=2, out_bstride=8,
                             rev_ptr=P, rev_pos=P, chunk_ptr=P, chunk_key=P, dv_workspace=P, **TAIL),
}
ALL = tuple(ENTRIES)
FWD = tuple(e for e in ALL if e.endswith("_fwd"))
BWD = tuple(e for e in ALL if e.endswith("_bwd"))
RAG = tuple(e for e in ALL if "ragged" in e)
RAG_FWD, RAG_BWD = RAG[:2], RAG[2:]
DIST = ("pit_distmat_fwd", "pit_distmat_bwd", "pit_distlist_fwd", "pit_distlist_bwd")
DIST_F, DIST_B = ("pit_distmat_fwd", "pit_distlist_fwd"), ("pit_distmat_bwd", "pit_distlist_bwd")
DMESH = ("pit_posatt_dmesh",)

# (entries, the arguments changed, the code)
TABLE = [
    # ---- null operands
    (ALL, dict(values=None), NULL),
    (ALL, dict(head=None), NULL),
    (ALL, dict(rowstat=None), NULL),
    (FWD, dict(stats=None), NULL),
    (FWD, dict(out=None), NULL),
    (BWD + DMESH, dict(d_out=None), NULL),
    (RAG + DMESH, dict(mesh_out=None), NULL),
    (RAG + DMESH, dict(mesh_in=None), NULL),
    (RAG_FWD, dict(rank_w=None), NULL),                              # a masked ragged layer interpolates per sample
    (("pit_posatt_ragged_fwd", "pit_posatt_ragged_bwd"), dict(len_out=None), NULL),
    (("pit_posatt_ragged_fwd", "pit_posatt_ragged_bwd"), dict(len_in=None), NULL),
    (RAG, dict(nbr_idx=P), NULL),                                    # lists without their counts
    (("pit_distmat_fwd", "pit_distmat_bwd"), dict(m=None), NULL),
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(idx=None), NULL),
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(sqd=None), NULL),
    (DMESH, dict(workspace=None), NULL),
    (BWD, dict(workspace=None), NULL),                               # d_head without a workspace
    (("pit_distmat_bwd",), dict(a_workspace=None), NULL),            # d_m without its workspace
    (DIST_B, dict(out=None), NULL),                                  # d_m / d_sqd without the forward's result
    (("pit_distlist_bwd",), dict(rev_pos=None), NULL),               # d_values without the transposed index
    (("pit_distlist_bwd",), dict(dv_workspace=None), NULL),
    # ---- sizes
    (ALL, dict(n_out=0), SIZE),
    (ALL, dict(n_in=0), SIZE),
    (ALL, dict(dim=0), SIZE),
    (ALL, dict(n_head=0), SIZE),
    (RAG + DMESH, dict(mesh_batch=0), SIZE),
    (DIST, dict(batch=0), SIZE),
    (RAG + DMESH, dict(space_dim=0), SIZE),
    (RAG, dict(space_dim=4), UNSUPPORTED),
    (DMESH, dict(space_dim=9), SIZE),
    (DMESH, dict(mesh_batch=3), SIZE),                               # neither shared nor one mesh per sample
    (RAG, dict(mesh_batch=65536), SIZE),
    (DIST, dict(batch=65536), UNSUPPORTED),
    (DMESH, dict(batch=65536, mesh_batch=1), UNSUPPORTED),
    (("pit_posatt_ragged_strided_fwd", "pit_posatt_ragged_strided_bwd"), dict(out_stride=3), SIZE),
    (("pit_posatt_ragged_strided_fwd", "pit_posatt_ragged_strided_bwd"), dict(in_stride=8), SIZE),
    (RAG, dict(nbr_idx=P, nbr_cnt=P), SIZE),                         # lists of capacity 0
    (("pit_distmat_fwd", "pit_distmat_bwd"), dict(ld_m=8), SIZE),
    (("pit_distmat_fwd", "pit_distmat_bwd"), dict(m_bstride=-1), SIZE),
    (("pit_distmat_fwd", "pit_distmat_bwd"), dict(m_bstride=35), SIZE),          # samples overlap
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(cap=0), SIZE),
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(ld=3), SIZE),
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(bstride=-1), SIZE),
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(bstride=15), SIZE),
    # ---- the values, out, d_out and d_values groups
    (DIST + DMESH, dict(ld_values=1), SIZE),
    (DIST + DMESH, dict(values_bstride=-1), SIZE),
    (DIST_F, dict(out_col0=-1), SIZE),
    (DIST_F, dict(ld_out=1), SIZE),
    (DIST_F, dict(out_col0=1), SIZE),                                # the head columns no longer fit in ld_out
    (DIST_F, dict(out_bstride=-1), SIZE),
    (RAG_FWD + DIST_F, dict(copy_inputs=1), SIZE),                   # n_out != n_in
    (DIST_F, dict(copy_inputs=1, n_in=4), SIZE),                     # self attention, but no room for the copied columns
    (DIST_B + DMESH, dict(out_col0=-1), SIZE),
    (DIST_B + DMESH, dict(ld_dout=1), SIZE),
    (DIST_B + DMESH, dict(dout_bstride=-1), SIZE),
    (RAG_BWD + DIST_B, dict(add_residual=1), SIZE),                  # n_out != n_in
    (DIST_B, dict(add_residual=1, n_in=4), SIZE),
    (DIST_B, dict(ld_dvalues=1), SIZE),
    (DIST_B, dict(dvalues_bstride=-1), SIZE),
    (DIST_B, dict(d_values=None, d_head=None, ld_out=1), SIZE),      # d_m / d_sqd alone: the forward's result too narrow
    (DIST_B, dict(d_values=None, d_head=None, out_bstride=-1), SIZE),
    # ---- the math mode
    (RAG + DIST, dict(math_mode=1), UNSUPPORTED),
    (DMESH, dict(metric=1), UNSUPPORTED),                            # periodic: refused
    (DMESH, dict(metric=3), -3),                                     # PIT_ERR_METRIC
    # ---- grid limits: the ragged entries answer PIT_ERR_SIZE, the others PIT_ERR_UNSUPPORTED
    (RAG, dict(n_head=65536, dim=1), SIZE),
    (RAG, dict(n_head=256, dim=256 * 255 + 1), SIZE),
    (("pit_distmat_fwd",), dict(n_head=65536, dim=1, ld_values=1), UNSUPPORTED),
    (("pit_distmat_fwd",), dict(n_head=256, dim=256 * 255 + 1, ld_values=256 * 255 + 1), UNSUPPORTED),
    (("pit_distmat_bwd",), dict(n_head=65536, dim=1, ld_dout=65536), UNSUPPORTED),
    (("pit_distlist_fwd",), dict(n_head=65536, dim=1), UNSUPPORTED),
    (("pit_distlist_bwd",), dict(n_head=65536, dim=1, ld_dout=65536), UNSUPPORTED),
    (("pit_distlist_fwd",), dict(dim=65536 * 256, ld_values=65536 * 256, n_in=1), UNSUPPORTED),
    (DMESH, dict(n_head=65536, dim=1, ld_dout=65536), UNSUPPORTED),
    (("pit_distlist_fwd", "pit_distlist_bwd"), dict(n_out=1 << 20, cap=1 << 11, ld=1 << 11), UNSUPPORTED),
    # ---- a buffer descriptor over PIT_MAX_BUFFER_BYTES
    (DIST + DMESH, dict(ld_values=BIG), UNSUPPORTED),
    (DIST_B + DMESH, dict(ld_dout=BIG), UNSUPPORTED),
    (DMESH, dict(values_bstride=BIG), UNSUPPORTED),                  # (one descriptor over the whole batch there)
    (("pit_distmat_fwd", "pit_distmat_bwd"), dict(ld_m=BIG), UNSUPPORTED),
    (("pit_distlist_fwd",), dict(ld_out=BIG), UNSUPPORTED),
    (("pit_distlist_bwd",), dict(d_values=None, d_head=None, ld_out=BIG), UNSUPPORTED),
]
ROWS = [(entry, changed, code) for entries, changed, code in TABLE for entry in entries]


def test_the_table_reaches_every_entry():
    assert {entry for entry, _, _ in ROWS} == set(ENTRIES)
    for entry, changed, _ in ROWS:
        assert set(changed) <= set(ENTRIES[entry]), (entry, changed)


@pytest.mark.parametrize("entry", ALL)
def test_entries_refuse_bad_arguments_before_any_launch(entry):
    from position_induced_transformer_amd import _lib
    fn = getattr(_lib.lib(), entry)
    base = ENTRIES[entry]
    assert len(base) == len(_lib.SIGNATURES[entry]), entry          # the table's argument order is the header's
    rows = [(changed, code) for e, changed, code in ROWS if e == entry]
    assert rows
    for changed, code in rows:
        assert fn(*{**base, **changed}.values()) == code, (entry, changed)
