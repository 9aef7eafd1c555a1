"""kc_ctg_index_build / kc_ctg_index_clear / kc_align_reads reject a NULL context and bad arguments before they touch a
device, and the record and the two statistics structs have the layout the header states (no GPU needed)."""
import ctypes as C

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import align_model as M


def test_index_build_null_checks():
    L = pkg.lib()
    st = _lib.kc_ctg_index_stats(contigs=7)
    offs = np.zeros(1, dtype=np.uint64)
    assert L.kc_ctg_index_build(None, None, 0, offs.ctypes.data, 0, 0, C.byref(st)) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_ctg_index_build(None, None, 0, None, 0, 0, None) == _lib.KC_ERR_INVALID_ARG
    assert st.contigs == 7  # nothing is written through the pointers of a call without a context
    assert L.kc_ctg_index_clear(None) == _lib.KC_ERR_INVALID_ARG


def test_align_reads_null_checks():
    L = pkg.lib()
    na, st = C.c_uint64(7), _lib.kc_align_stats(reads=7)
    offs = np.zeros(1, dtype=np.uint64)
    assert L.kc_align_reads(None, None, offs.ctypes.data, 0, 0, 1, 0, None, 0, None, C.byref(na), C.byref(st)) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_align_reads(None, None, None, 0, 0, 1, 0, None, 0, None, None, None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_align_reads(None, None, None, 0, 0, 0, 0, None, 0, None, C.byref(na), None) == _lib.KC_ERR_INVALID_ARG
    assert (na.value, st.reads) == (7, 7)


def test_record_and_stats_layout():
    assert C.sizeof(_lib.kc_read_aln) == 32
    assert [(n, C.sizeof(t)) for n, t in _lib.kc_read_aln._fields_] == [("read", 4), ("ctg", 4), ("cstart", 4), ("cstop", 4), ("rstart", 2),
                                                                        ("rstop", 2), ("mismatches", 2), ("seeds", 2), ("orient", 1),
                                                                        ("pad", 7)]
    assert _lib.kc_read_aln.orient.offset == 24
    assert C.sizeof(_lib.kc_ctg_index_stats) == 40
    assert [(n, C.sizeof(t)) for n, t in _lib.kc_ctg_index_stats._fields_] == [(n, 8) for n in M.INDEX_STATS]
    assert C.sizeof(_lib.kc_align_stats) == 56
    assert [(n, C.sizeof(t)) for n, t in _lib.kc_align_stats._fields_] == [(n, 8) for n in M.ALIGN_STATS]
    # the numpy view of a record, in the package and in the model, is the C struct
    for dt in (kcount.ALN_DTYPE, M.ALN_DTYPE):
        assert dt.itemsize == 32
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(_lib.kc_read_aln, n).offset) for n, _ in _lib.kc_read_aln._fields_]
    assert _lib.KC_ALIGN_MAX_READ_LEN == M.MAX_READ_LEN == 1024
