"""kc_scaffold is exported, its parameters, records and statistics have the layout the header states, and every range that
needs no device is refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import scaffold_model as M
from test_scaffold_model import BAD_PARAMS

GOOD = dict(min_splints=1, min_spans=2, max_second_permille=0, overlap_slack=0, flags=0)


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_scaffold" in _lib.SYMBOLS
    f = L.kc_scaffold
    assert f.restype is C.c_int and len(f.argtypes) == 14
    assert callable(kcount.KmerCounter.scaffolds) and callable(kcount.KmerCounter.scaffold_strings)
    assert L.kc_abi_version() == 1


def test_layouts():
    sizes = (C.sizeof(_lib.kc_scaf_params), C.sizeof(_lib.kc_scaffold_rec), C.sizeof(_lib.kc_scaf_member), C.sizeof(_lib.kc_scaf_stats))
    assert sizes == (32, 32, 16, 160)
    assert [n for n, _ in _lib.kc_scaf_params._fields_] == list(GOOD) + ["reserved"] and GOOD == M.DEFAULTS
    assert [getattr(_lib.kc_scaf_params, n).offset for n, _ in _lib.kc_scaf_params._fields_] == [0, 4, 8, 12, 16, 20]
    want = [("first_member", 0), ("n_members", 4), ("len", 8), ("n_bases", 12), ("overlap_bases", 16), ("flags", 20), ("pad", 24)]
    assert [(n.replace("reserved", "pad"), getattr(_lib.kc_scaffold_rec, n).offset) for n, _ in _lib.kc_scaffold_rec._fields_] == want
    for dt in (kcount.SCAFFOLD_DTYPE, M.SCAFFOLD_DTYPE):
        assert dt.itemsize == 32 and [(n, dt.fields[n][1]) for n in dt.names] == want
    want = [("ctg", 0), ("join", 4), ("out_pos", 8), ("orient", 12), ("pad", 13)]
    assert [(n.replace("reserved", "pad"), getattr(_lib.kc_scaf_member, n).offset) for n, _ in _lib.kc_scaf_member._fields_] == want
    for dt in (kcount.MEMBER_DTYPE, M.MEMBER_DTYPE):
        assert dt.itemsize == 16 and [(n, dt.fields[n][1]) for n in dt.names] == want and dt.fields["join"][0].kind == "i"
    assert [n for n, _ in _lib.kc_scaf_stats._fields_] == list(M.SCAF_STATS) + ["reserved"]
    assert [getattr(_lib.kc_scaf_stats, n).offset for n in M.SCAF_STATS] == list(range(0, 136, 8))
    assert (_lib.KC_SCAF_MAX_SLACK, _lib.KC_SCAF_CIRCULAR) == (M.MAX_SLACK, M.CIRCULAR) == (64, 1)
    assert M.LINK_DTYPE == kcount.LINK_DTYPE
    sig = inspect.signature(kcount.KmerCounter.scaffolds).parameters
    assert {n: sig[n].default for n in GOOD if n != "flags"} == {n: v for n, v in M.DEFAULTS.items() if n != "flags"}


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    links = np.zeros(2, dtype=kcount.LINK_DTYPE)
    seqs = np.full(64, 0xAB, dtype=np.uint8)
    offs = np.full(4, 0xABAB, dtype=np.uint64)
    scafs = np.full(64, 0xAB, dtype=np.uint8)
    members = np.full(64, 0xAB, dtype=np.uint8)
    cm = np.full(4, 0xABAB, dtype=np.uint32)
    ns, nb = C.c_uint64(7), C.c_uint64(7)
    st = _lib.kc_scaf_stats(contigs=7, longest=7)

    def call(reserved=(0, 0, 0), **kw):
        p = _lib.kc_scaf_params(**dict(GOOD, **kw))
        p.reserved[:] = reserved
        return L.kc_scaffold(None, links.ctypes.data, 2, 0, C.byref(p), seqs.ctypes.data, 64, offs.ctypes.data, scafs.ctypes.data,
                             members.ctypes.data, cm.ctypes.data, C.byref(ns), C.byref(nb), C.byref(st))

    bad = BAD_PARAMS + [(dict(min_splints=0, min_spans=0), "kc_scaffold: min_splints 0, min_spans 0 below 1"),
                        (dict(max_second_permille=0xFFFFFFFF), "kc_scaffold: max_second_permille 4294967295 over 1000"),
                        (dict(overlap_slack=0xFFFFFFFF), "kc_scaffold: overlap_slack 4294967295 over 64"),
                        (dict(flags=0x80000000), "kc_scaffold: unknown flags 0x80000000")]
    for kw, text in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert text.encode() in L.kc_last_error(), (kw, L.kc_last_error())
        try:
            M.scaffold(["ACGT"], M.records([]), **kw)
        except M.BadArg as e:
            assert str(e).encode() in L.kc_last_error(), (str(e), L.kc_last_error())  # the model names the same values
        else:
            raise AssertionError("the model took %r" % (kw,))
    assert call(reserved=(0, 4, 0)) == _lib.KC_ERR_INVALID_ARG and b"kc_scaffold: unknown flags 0x4" in L.kc_last_error()
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    for kw in (dict(min_splints=1, min_spans=1), dict(min_splints=0xFFFFFFFF, min_spans=0xFFFFFFFF), dict(max_second_permille=1000),
               dict(overlap_slack=64), {}):
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert b"unknown flags 0x4" in L.kc_last_error(), kw
    # the parameters and the two counts are required
    p = _lib.kc_scaf_params(**GOOD)
    assert L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, C.byref(ns), C.byref(nb), None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_scaffold(None, None, 0, 0, C.byref(p), None, 0, None, None, None, None, None, C.byref(nb), None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_scaffold(None, None, 0, 0, C.byref(p), None, 0, None, None, None, None, C.byref(ns), None, None) == _lib.KC_ERR_INVALID_ARG
    assert (ns.value, nb.value, st.contigs, st.longest) == (7, 7, 7, 7)
    assert (seqs == 0xAB).all() and (offs == 0xABAB).all() and (scafs == 0xAB).all() and (members == 0xAB).all() and (cm == 0xABAB).all()
