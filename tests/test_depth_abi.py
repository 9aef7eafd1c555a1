"""kc_ctg_index_info, kc_aln_depths and kc_pair_inserts are exported, their records and statistics have the layout the
header states, and the ranges that need no device are refused in front of the context, by the values kc_last_error names
(no GPU needed)."""
import ctypes as C

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import depth_model as D


def test_symbols_are_exported():
    L = pkg.lib()
    for name, nargs in (("kc_ctg_index_info", 3), ("kc_aln_depths", 12), ("kc_pair_inserts", 12)):
        assert name in _lib.SYMBOLS
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs
    for m in ("contig_index_info", "aln_depths", "pair_inserts"):
        assert callable(getattr(kcount.KmerCounter, m))


def test_record_and_stats_layout():
    assert C.sizeof(_lib.kc_ctg_depth) == 32 and C.sizeof(_lib.kc_pair_rec) == 16
    assert [getattr(_lib.kc_ctg_depth, n).offset for n, _ in _lib.kc_ctg_depth._fields_] == [0, 8, 12, 16, 20, 24, 28]
    assert [getattr(_lib.kc_pair_rec, n).offset for n, _ in _lib.kc_pair_rec._fields_] == [0, 4, 8, 12, 13]
    for dt, st in ((kcount.CTG_DEPTH_DTYPE, _lib.kc_ctg_depth), (D.CTG_DEPTH_DTYPE, _lib.kc_ctg_depth), (kcount.PAIR_DTYPE, _lib.kc_pair_rec),
                   (D.PAIR_DTYPE, _lib.kc_pair_rec)):
        assert dt.itemsize == C.sizeof(st)
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    assert C.sizeof(_lib.kc_depth_stats) == 9 * 8 and [n for n, _ in _lib.kc_depth_stats._fields_] == list(D.DEPTH_STATS)
    assert C.sizeof(_lib.kc_insert_stats) == 11 * 8
    assert [(n, getattr(_lib.kc_insert_stats, n).offset) for n, _ in _lib.kc_insert_stats._fields_] == [
        ("pairs", 0), ("cls", 8), ("insert_sum", 64), ("insert_sq_sum", 72), ("reads_with_best", 80)]
    assert _lib.KC_DEPTH_MAX_EDGE == D.MAX_EDGE == 1024 and _lib.KC_INSERT_MAX == D.INSERT_MAX == 65535
    assert (_lib.KC_DEPTH_BEST_ONLY, _lib.KC_DEPTH_PER_CONTIG) == (D.BEST_ONLY, D.PER_CONTIG) == (1, 2)
    assert (_lib.KC_PAIR_NONE, _lib.KC_PAIR_ONE, _lib.KC_PAIR_DIFF_CTG, _lib.KC_PAIR_SAME_ORIENT, _lib.KC_PAIR_EVERTED, _lib.KC_PAIR_TOO_LONG,
            _lib.KC_PAIR_PROPER) == (D.PAIR_NONE, D.PAIR_ONE, D.PAIR_DIFF_CTG, D.PAIR_SAME_ORIENT, D.PAIR_EVERTED, D.PAIR_TOO_LONG,
                                     D.PAIR_PROPER) == tuple(range(7))


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    alns = np.zeros(1, dtype=kcount.GAP_ALN_DTYPE)
    depths = np.full(8, 0xABAB, dtype=np.uint16)
    ctgs = np.full(64, 0xAB, dtype=np.uint8)
    dst = _lib.kc_depth_stats(records=7, saturated=7)

    def depth(edge_clip=0, flags=0):
        return L.kc_aln_depths(None, alns.ctypes.data, 1, 0, 0, 0, 0, edge_clip, flags, depths.ctypes.data, ctgs.ctypes.data, C.byref(dst))

    assert depth(edge_clip=1025) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_aln_depths: edge_clip 1025 over 1024 or unknown flags 0x0" in L.kc_last_error()
    assert depth(flags=4) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_aln_depths: edge_clip 0 over 1024 or unknown flags 0x4" in L.kc_last_error()
    assert depth(flags=0x80000001) == _lib.KC_ERR_INVALID_ARG
    assert b"unknown flags 0x80000001" in L.kc_last_error()
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    assert depth(edge_clip=1024, flags=3) == _lib.KC_ERR_INVALID_ARG
    assert b"unknown flags 0x80000001" in L.kc_last_error()
    assert (dst.records, dst.saturated) == (7, 7) and (depths == 0xABAB).all() and (ctgs == 0xAB).all()

    offs = np.zeros(4, dtype=np.uint64)
    hist = np.full(8, 0xAB, dtype=np.uint8)
    pairs = np.full(32, 0xAB, dtype=np.uint8)
    ist = _lib.kc_insert_stats(pairs=7, reads_with_best=7)

    def inserts(nreads=2, max_insert=1000):
        return L.kc_pair_inserts(None, offs.ctypes.data, nreads, alns.ctypes.data, 1, 0, 0, 0, max_insert, hist.ctypes.data, pairs.ctypes.data,
                                 C.byref(ist))

    assert inserts(max_insert=0) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_pair_inserts: max_insert 0 outside 1 .. 65535" in L.kc_last_error()
    assert inserts(max_insert=65536) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_pair_inserts: max_insert 65536 outside 1 .. 65535" in L.kc_last_error()
    assert inserts(nreads=3) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_pair_inserts: 3 reads are no pairs" in L.kc_last_error()
    for ok in (1, 65535):
        assert inserts(max_insert=ok) == _lib.KC_ERR_INVALID_ARG
        assert b"3 reads are no pairs" in L.kc_last_error()
    assert (ist.pairs, ist.reads_with_best) == (7, 7) and (hist == 0xAB).all() and (pairs == 0xAB).all()
    assert L.kc_ctg_index_info(None, None, None) == _lib.KC_ERR_INVALID_ARG
