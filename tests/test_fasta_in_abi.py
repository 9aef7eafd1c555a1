"""kc_fasta_to_block is exported, its parameters, statistics and record have the layout the header states, and every range
that needs no device is refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import fasta_in_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_fasta_to_block" in _lib.SYMBOLS
    assert L.kc_fasta_to_block.restype is C.c_int and len(L.kc_fasta_to_block.argtypes) == 15
    for name in ("fasta_to_block", "load_contigs"):
        assert callable(getattr(kcount.KmerCounter, name))
    assert pkg.FASTA_REC_DTYPE == M.REC_DTYPE and pkg.FASTA_REC_DTYPE.itemsize == 32
    assert L.kc_abi_version() == 1


def test_layouts_and_constants():
    assert (C.sizeof(_lib.kc_fasta_in_params), C.sizeof(_lib.kc_fasta_in_stats), C.sizeof(_lib.kc_fasta_rec)) == (32, 128, 32)
    want = [("flags", 0), ("default_depth", 4), ("reserved", 8)]
    assert [(n, getattr(_lib.kc_fasta_in_params, n).offset) for n, _ in _lib.kc_fasta_in_params._fields_] == want
    assert [n for n, _ in _lib.kc_fasta_in_stats._fields_] == list(M.STATS) + ["reserved"]
    assert [getattr(_lib.kc_fasta_in_stats, n).offset for n, _ in _lib.kc_fasta_in_stats._fields_] == list(range(0, 88, 8))
    want = [("hdr_pos", 0), ("hdr_len", 8), ("seq_lines", 12), ("id", 16), ("depth", 24), ("flags", 28)]
    assert [(n, getattr(_lib.kc_fasta_rec, n).offset) for n, _ in _lib.kc_fasta_rec._fields_] == want
    assert [(n, M.REC_DTYPE.fields[n][1]) for n in M.REC_DTYPE.names] == want
    header = open(os.path.join(ROOT, "include", "kcount_mi355.h")).read()
    for name, value in (("PARTIAL", M.PARTIAL), ("STRICT", M.STRICT), ("HAS_ID", M.HAS_ID), ("HAS_DEPTH", M.HAS_DEPTH), ("LOWERED", M.LOWERED),
                        ("RECODED", M.RECODED)):
        assert getattr(_lib, "KC_FASTA_" + name) == value and re.search(r"#define KC_FASTA_%s %du\b" % (name, value), header), name
    assert _lib.KC_FASTA_HDR_SCAN == M.HDR_SCAN == 256 and re.search(r"#define KC_FASTA_HDR_SCAN 256\b", header)
    for struct, size in (("kc_fasta_in_params", 32), ("kc_fasta_in_stats", 128), ("kc_fasta_rec", 32)):
        assert re.search(r"typedef struct %s \{ /\* %d bytes \*/" % (struct, size), header), struct
    sig = inspect.signature(kcount.KmerCounter.fasta_to_block).parameters
    assert list(sig)[1:] == ["text", "partial", "strict", "default_depth", "with_depths", "with_records"]
    assert [sig[n].default for n in list(sig)[2:]] == [False, False, 0, False, True]
    sig = inspect.signature(kcount.KmerCounter.load_contigs).parameters
    assert list(sig)[1:] == ["path_or_fileobj", "window_bytes", "strict", "default_depth", "with_depths", "with_records"]
    assert [sig[n].default for n in list(sig)[2:]] == [256 << 20, False, 0, False, True]


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    text = np.frombuffer(b">a\nACGT\n", dtype=np.uint8).copy()
    seqs = np.full(64, 0xA5, dtype=np.uint8)
    offsets = np.full(8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    depths = np.full(64, 0xA5A5, dtype=np.uint16)
    recs = np.full(32, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    nc, nb, cons = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    st = _lib.kc_fasta_in_stats(lines=7, with_depth=7)

    def reserved(at, value):
        r = (C.c_uint32 * 6)()
        r[at] = value
        return r

    def call(p=True, n=nc, b=nb, **kw):
        prm = _lib.kc_fasta_in_params(**kw)
        return L.kc_fasta_to_block(None, text.ctypes.data, len(text), 0, C.byref(prm) if p else None, seqs.ctypes.data, 64, offsets.ctypes.data, 7,
                                   depths.ctypes.data, recs.ctypes.data, n and C.byref(n), b and C.byref(b), C.byref(cons), C.byref(st))

    bad = [(lambda: call(flags=4), "kc_fasta_to_block: unknown flags 0x4"),
           (lambda: call(flags=0x80000003), "kc_fasta_to_block: unknown flags 0x80000000"),
           (lambda: call(default_depth=65536), "kc_fasta_to_block: default_depth 65536 over 65535"),
           (lambda: call(default_depth=0xFFFFFFFF), "kc_fasta_to_block: default_depth 4294967295 over 65535"),
           (lambda: call(reserved=reserved(0, 1)), "kc_fasta_to_block: reserved[0] is 1, not zero"),
           (lambda: call(reserved=reserved(5, 9)), "kc_fasta_to_block: reserved[5] is 9, not zero"),
           (lambda: call(p=False), "kc_fasta_to_block: params is NULL"),
           (lambda: call(n=None), "kc_fasta_to_block: n_ctgs is NULL"),
           (lambda: call(b=None), "kc_fasta_to_block: nbytes is NULL")]
    for f, message in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)  # leaves another text behind
        assert f() == _lib.KC_ERR_INVALID_ARG, message
        assert message.encode() in L.kc_last_error(), (message, L.kc_last_error())
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    marker = L.kc_last_error()
    for f in (lambda: call(), lambda: call(flags=3, default_depth=65535), lambda: call(flags=1), lambda: call(flags=2, default_depth=1)):
        assert f() == _lib.KC_ERR_INVALID_ARG
        assert L.kc_last_error() == marker
    assert (nc.value, nb.value, cons.value, st.lines, st.with_depth) == (7, 7, 7, 7, 7)
    assert (seqs == 0xA5).all() and (offsets == 0xA5A5A5A5A5A5A5A5).all() and (depths == 0xA5A5).all() and (recs == 0xA5A5A5A5A5A5A5A5).all()


def test_the_wrappers_refuse_before_any_library_call():
    import pytest
    kc = object.__new__(kcount.KmerCounter)  # no context: a call into the library would fail on the missing handle
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match="default_depth"):
            kc.fasta_to_block(b">a\nAC\n", default_depth=bad)
        with pytest.raises(ValueError, match="default_depth"):
            kc.load_contigs("nowhere.fa", default_depth=bad)
    with pytest.raises(ValueError, match="window_bytes"):
        kc.load_contigs("nowhere.fa", window_bytes=0)
    with pytest.raises(ValueError, match="uint8"):
        kc.fasta_to_block(np.zeros(4, dtype=np.uint16))
