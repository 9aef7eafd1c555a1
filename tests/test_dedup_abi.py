"""kc_ctg_dedup is exported, its parameters, records and statistics have the layout the header states, and every range that
needs no device is refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import dedup_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_ctg_dedup" in _lib.SYMBOLS
    assert L.kc_ctg_dedup.restype is C.c_int and len(L.kc_ctg_dedup.argtypes) == 16
    for name in ("dedup_contigs", "dedup_strings"):
        assert callable(getattr(kcount.KmerCounter, name))
    assert L.kc_abi_version() == 1


def test_layouts_and_constants():
    assert (C.sizeof(_lib.kc_dedup_params), C.sizeof(_lib.kc_dedup_rec), C.sizeof(_lib.kc_dedup_stats)) == (32, 32, 128)
    want = [("max_mismatches", 0), ("flags", 4), ("max_candidates", 8), ("reserved", 16)]
    assert [(n, getattr(_lib.kc_dedup_params, n).offset) for n, _ in _lib.kc_dedup_params._fields_] == want
    want = [("status", 0), ("container", 4), ("pos", 8), ("mismatches", 12), ("new_index", 16), ("len", 20), ("absorbed", 24), ("orient", 28),
            ("flags", 29), ("reserved", 30)]
    assert [(n, getattr(_lib.kc_dedup_rec, n).offset) for n, _ in _lib.kc_dedup_rec._fields_] == want
    for dtype in (M.REC_DTYPE, kcount.DEDUP_DTYPE):
        assert dtype.itemsize == 32 and [(n, dtype.fields[n][1]) for n in dtype.names] == want[:-1] + [("pad", 30)]
    assert [n for n, _ in _lib.kc_dedup_stats._fields_] == list(M.STATS) + ["reserved"]
    assert [getattr(_lib.kc_dedup_stats, n).offset for n, _ in _lib.kc_dedup_stats._fields_] == list(range(0, 120, 8))
    assert _lib.KC_DEDUP_DUPLICATES_ONLY == M.DUPLICATES_ONLY == 1 and _lib.KC_DEDUP_UNANCHORED == M.UNANCHORED == 1
    assert (_lib.KC_DEDUP_KEPT, _lib.KC_DEDUP_DUPLICATE, _lib.KC_DEDUP_CONTAINED) == (M.KEPT, M.DUPLICATE, M.CONTAINED) == (0, 1, 2)
    assert _lib.KC_DEDUP_NONE == M.NONE == 0xFFFFFFFF
    header = open(os.path.join(ROOT, "include", "kcount_mi355.h")).read()
    for name, value in (("DUPLICATES_ONLY", 1), ("KEPT", 0), ("DUPLICATE", 1), ("CONTAINED", 2), ("UNANCHORED", 1)):
        assert re.search(r"#define KC_DEDUP_%s %du\b" % (name, value), header), name
    assert "0: 2^26" in header and M.DEFAULT_MAX_CANDIDATES == 1 << 26
    sig = inspect.signature(kcount.KmerCounter.dedup_contigs).parameters
    assert list(sig)[1:] == ["seqs", "offsets", "depths", "max_mismatches", "duplicates_only", "max_candidates"]
    assert [sig[n].default for n in list(sig)[3:]] == [None, 0, False, 0]
    sig = inspect.signature(M.dedup).parameters
    assert [(n, sig[n].default) for n in ("max_mismatches", "duplicates_only", "max_candidates")] == [("max_mismatches", 0), ("duplicates_only", False),
                                                                                                      ("max_candidates", 0)]


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    seqs, offsets = M.block(["ACGT", "GGNCA", "T"])
    depths = np.full(len(seqs), 3, dtype=np.uint16)
    out = np.full(64, 0xA5, dtype=np.uint8)
    out_d = np.full(64, 0xA5A5, dtype=np.uint16)
    out_o = np.full(8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    recs = np.full(4 * 32, 0xA5, dtype=np.uint8)
    nk, nb = C.c_uint64(7), C.c_uint64(7)
    st = _lib.kc_dedup_stats(contigs=7, longest_removed=7)

    def dedup(params=True, n_out=nk, nbytes_out=nb, **kw):
        p = _lib.kc_dedup_params(**kw)
        return L.kc_ctg_dedup(None, seqs.ctypes.data, len(seqs), offsets.ctypes.data, 3, depths.ctypes.data, 0, C.byref(p) if params else None,
                              recs.ctypes.data, out.ctypes.data, 64, out_o.ctypes.data, out_d.ctypes.data, n_out and C.byref(n_out),
                              nbytes_out and C.byref(nbytes_out), C.byref(st))

    def reserved(at, value):
        r = (C.c_uint32 * 4)()
        r[at] = value
        return r

    bad = [(lambda: dedup(flags=2), "kc_ctg_dedup: unknown flags 0x2"),
           (lambda: dedup(flags=0x80000001), "kc_ctg_dedup: unknown flags 0x80000000"),
           (lambda: dedup(reserved=reserved(0, 1)), "kc_ctg_dedup: reserved[0] is 1, not zero"),
           (lambda: dedup(reserved=reserved(3, 9)), "kc_ctg_dedup: reserved[3] is 9, not zero"),
           (lambda: dedup(params=False), "kc_ctg_dedup: params is NULL"),
           (lambda: dedup(n_out=None), "kc_ctg_dedup: n_out is NULL"),
           (lambda: dedup(nbytes_out=None), "kc_ctg_dedup: nbytes_out is NULL")]
    for call, message in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)  # leaves another text behind
        assert call() == _lib.KC_ERR_INVALID_ARG, message
        assert message.encode() in L.kc_last_error(), (message, L.kc_last_error())
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    marker = L.kc_last_error()
    good = [lambda: dedup(), lambda: dedup(max_mismatches=0xFFFFFFFF, flags=1, max_candidates=0xFFFFFFFFFFFFFFFF), lambda: dedup(max_candidates=1)]
    for call in good:
        assert call() == _lib.KC_ERR_INVALID_ARG
        assert L.kc_last_error() == marker
    assert (nk.value, nb.value, st.contigs, st.longest_removed) == (7, 7, 7, 7)
    assert (out == 0xA5).all() and (out_d == 0xA5A5).all() and (out_o == 0xA5A5A5A5A5A5A5A5).all() and (recs == 0xA5).all()
