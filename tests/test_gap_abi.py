"""kc_align_gapped rejects a NULL context, scores or output and scores, pad or flags out of range before it touches a
device, and the record and the statistics struct have the layout the header states (no GPU needed)."""
import ctypes as C

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import gap_model as G


def test_symbol_is_exported():
    assert "kc_align_gapped" in _lib.SYMBOLS
    f = pkg.lib().kc_align_gapped
    assert f.restype is C.c_int and len(f.argtypes) == 12


def test_null_and_range_checks_write_nothing():
    L = pkg.lib()
    st = _lib.kc_gap_stats(records=7, score_sum=7)
    out = np.full(64, 0xAB, dtype=np.uint8)
    alns = np.zeros(1, dtype=kcount.ALN_DTYPE)
    offs = np.zeros(2, dtype=np.uint64)
    good = _lib.kc_aln_scores(2, 3, 5, 2, 1)

    def call(ctx, scores, po, pad=16, flags=0):
        return L.kc_align_gapped(ctx, None, offs.ctypes.data, 1, alns.ctypes.data, 1, 0, pad, scores, flags, po, C.byref(st))

    assert call(None, C.byref(good), out.ctypes.data) == _lib.KC_ERR_INVALID_ARG
    assert call(None, None, out.ctypes.data) == _lib.KC_ERR_INVALID_ARG
    assert call(None, C.byref(good), None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_align_gapped(None, None, None, 0, None, 0, 0, 0, None, 0, None, None) == _lib.KC_ERR_INVALID_ARG
    # The ranges are checked in front of the context, so a NULL one reaches them: kc_last_error names the refused values,
    # which no other path writes.  With a context they run in test_gpu_gap_align.py.
    for bad in ((0, 3, 5, 2, 1), (10, 3, 5, 2, 1), (2, 10, 5, 2, 1), (2, 3, 5, 6, 1), (2, 3, 5, 0, 1), (2, 3, 10, 2, 1), (2, 3, 5, 2, 10)):
        assert call(None, C.byref(_lib.kc_aln_scores(*bad)), out.ctypes.data) == _lib.KC_ERR_INVALID_ARG
        assert ("scores %d %d %d %d %d outside" % bad).encode() in L.kc_last_error()
    assert call(None, C.byref(good), out.ctypes.data, pad=_lib.KC_GAP_MAX_PAD + 1) == _lib.KC_ERR_INVALID_ARG
    assert b"pad 1025 over 1024" in L.kc_last_error()
    assert call(None, C.byref(good), out.ctypes.data, flags=2) == _lib.KC_ERR_INVALID_ARG
    assert b"pad 16 over 1024 or unknown flags 0x2" in L.kc_last_error()
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    for ok in ((2, 3, 5, 2, 1), (1, 0, 1, 1, 0), (9, 9, 9, 9, 9)):
        assert call(None, C.byref(_lib.kc_aln_scores(*ok)), out.ctypes.data, pad=_lib.KC_GAP_MAX_PAD, flags=1) == _lib.KC_ERR_INVALID_ARG
        assert b"unknown flags 0x2" in L.kc_last_error()
    assert (st.records, st.score_sum) == (7, 7) and (out == 0xAB).all()  # nothing is written through any pointer
    assert tuple(getattr(good, n) for n, _ in good._fields_) == (2, 3, 5, 2, 1)


def test_record_and_stats_layout():
    assert C.sizeof(_lib.kc_gap_aln) == 32
    assert [(n, C.sizeof(t)) for n, t in _lib.kc_gap_aln._fields_] == [("read", 4), ("ctg", 4), ("cstart", 4), ("cstop", 4), ("rstart", 2),
                                                                       ("rstop", 2), ("score", 4), ("mismatches", 2), ("seeds", 2),
                                                                       ("orient", 1), ("kind", 1), ("pad", 2)]
    assert [getattr(_lib.kc_gap_aln, n).offset for n, _ in _lib.kc_gap_aln._fields_] == [0, 4, 8, 12, 16, 18, 20, 24, 26, 28, 29, 30]
    assert C.sizeof(_lib.kc_gap_stats) == 6 * 8
    assert [(n, C.sizeof(t)) for n, t in _lib.kc_gap_stats._fields_] == [(n, 8) for n in G.GAP_STATS]
    assert C.sizeof(_lib.kc_aln_scores) == 20
    assert [n for n, _ in _lib.kc_aln_scores._fields_] == ["match", "mismatch", "gap_open", "gap_ext", "ambiguity"]
    # the numpy view of a record, in the package and in the model, is the C struct
    for dt in (kcount.GAP_ALN_DTYPE, G.GAP_ALN_DTYPE):
        assert dt.itemsize == 32
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(_lib.kc_gap_aln, n).offset) for n, _ in _lib.kc_gap_aln._fields_]
    assert _lib.KC_GAP_MAX_PAD == G.MAX_PAD == 1024 and _lib.KC_GAP_ALWAYS_DP == 1
    assert (_lib.KC_GAP_EXACT, _lib.KC_GAP_DP, _lib.KC_GAP_NONE) == (G.KIND_EXACT, G.KIND_DP, G.KIND_NONE) == (0, 1, 2)
    assert kcount.BLASTN_ALN_SCORES == G.SCORES_BLASTN and kcount.ALTERNATE_ALN_SCORES == G.SCORES_ALTERNATE
