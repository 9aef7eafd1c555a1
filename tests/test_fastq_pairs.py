"""kc_fastq_pairs (paired FASTQ -> interleaved ASCII reads, host only) and the argument checks of kc_merge_pairs that
need no GPU."""
import ctypes as C

import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

R1 = b"@p0/1\nACGTN\n+\nIIII#\n@p1/1\nGGCa\n+\nI5I5\n"
R2 = b"@p0/2\nTTG\n+\n#II\n@p1/2\nCCRTA\n+\nIIIII\n"


def test_two_files_interleave_record_by_record():
    b, q, o = pkg.fastq_pairs(R1, R2)
    assert o.tolist() == [0, 5, 8, 12, 17]
    assert bytes(b) == b"ACGTN" + b"TTG" + b"GGCa" + b"CCRTA"
    assert bytes(q) == b"IIII#" + b"#II" + b"I5I5" + b"IIIII"


def test_interleaved_file_crlf_and_trailing_space():
    text = b"@p0/1\r\nACGTN \r\n+\r\nIIII#\t\r\n@p0/2\nTTG\n+\n#II\n"
    b, q, o = pkg.fastq_pairs(text)
    assert o.tolist() == [0, 5, 8]
    assert bytes(b) == b"ACGTNTTG" and bytes(q) == b"IIII##II"
    assert pkg.fastq_pairs(text + b"\n")[2].tolist() == [0, 5, 8]


def _call(t1, t2, cap=0, rcap=0, arrays=False):
    L = pkg.lib()
    n, nb = C.c_uint64(0), C.c_uint64(0)
    bases = np.zeros(max(cap, 1), np.uint8)
    quals = np.zeros(max(cap, 1), np.uint8)
    offs = np.zeros(rcap + 1, np.uint64)
    st = L.kc_fastq_pairs(t1, len(t1), t2, 0 if t2 is None else len(t2), bases.ctypes.data if arrays else None,
                          quals.ctypes.data if arrays else None, cap, offs.ctypes.data if arrays else None, rcap, C.byref(n), C.byref(nb))
    return st, n.value, nb.value


def test_size_query_and_capacity():
    st, n, nb = _call(R1, R2)
    assert st == _lib.KC_ERR_CAPACITY and (n, nb) == (4, 17)
    st, n, nb = _call(R1, R2, cap=16, rcap=4, arrays=True)
    assert st == _lib.KC_ERR_CAPACITY and (n, nb) == (4, 17)
    st, n, nb = _call(R1, R2, cap=17, rcap=4, arrays=True)
    assert st == _lib.KC_OK and (n, nb) == (4, 17)
    assert _call(b"", None) == (_lib.KC_OK, 0, 0)


def test_count_mismatch_and_odd_interleaved_count():
    one = b"@p0/1\nACGT\n+\nIIII\n"
    assert _call(R1, one)[0] == _lib.KC_ERR_INVALID_ARG
    assert _call(one, R2)[0] == _lib.KC_ERR_INVALID_ARG
    assert _call(R1 + one, None)[0] == _lib.KC_ERR_INVALID_ARG
    with pytest.raises(pkg.KcError):
        pkg.fastq_pairs(R1, one)


def test_bad_base_and_malformed_record():
    bad = b"@p0/2\nTTX\n+\n#II\n@p1/2\nCCRTA\n+\nIIIII\n"
    assert _call(R1, bad)[0] == _lib.KC_ERR_BAD_BASE
    assert _call(R1, b"@p0/2\nTTG\n+\n#I\n")[0] == _lib.KC_ERR_INVALID_ARG
    assert _call(b"p0/1\nACGT\n+\nIIII\n@x\nA\n+\nI\n", None)[0] == _lib.KC_ERR_INVALID_ARG


def test_merge_pairs_needs_a_context():
    L = pkg.lib()
    n, nb = C.c_uint64(0), C.c_uint64(0)
    st = _lib.kc_merge_stats()
    b = np.zeros(8, np.uint8)
    o = np.array([0, 4, 8], np.uint64)
    assert L.kc_merge_pairs(None, b.ctypes.data, b.ctypes.data, o.ctypes.data, 1, 0, 0, None, 0, None, 0, C.byref(n), C.byref(nb),
                            C.byref(st)) == _lib.KC_ERR_INVALID_ARG
