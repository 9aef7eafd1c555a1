"""kc_fastq_text is exported, its parameters have the layout the header states, and every range that needs no device is
refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import fastq_out_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_fastq_text" in _lib.SYMBOLS
    assert L.kc_fastq_text.restype is C.c_int and len(L.kc_fastq_text.argtypes) == 15
    for name in ("fastq_text", "write_fastq", "write_fastq_pairs"):
        assert callable(getattr(kcount.KmerCounter, name))
    assert L.kc_abi_version() == 1


def test_layout_constants_and_signatures():
    assert C.sizeof(_lib.kc_fastq_out_params) == 64
    want = [("flags", 0), ("prefix_len", 4), ("first_id", 8), ("prefix", 16), ("reserved", 48)]
    assert [(n, getattr(_lib.kc_fastq_out_params, n).offset) for n, _ in _lib.kc_fastq_out_params._fields_] == want
    assert (_lib.KC_FASTQ_OUT_PACKED, _lib.KC_FASTQ_OUT_PAIRED, _lib.KC_FASTQ_OUT_CHECK) == (M.PACKED, M.PAIRED, M.CHECK) == (1, 2, 4)
    assert _lib.KC_FASTQ_OUT_MAX_PREFIX == M.MAX_PREFIX == 32
    header = open(os.path.join(ROOT, "include", "kcount_mi355.h")).read()
    for name, value in (("PACKED", 1), ("PAIRED", 2), ("CHECK", 4)):
        assert re.search(r"#define KC_FASTQ_OUT_%s +%du\b" % (name, value), header), name
    assert re.search(r"#define KC_FASTQ_OUT_MAX_PREFIX 32\b", header)
    assert re.search(r"typedef struct kc_fastq_out_params \{ /\* 64 bytes \*/\s+uint32_t flags, prefix_len;\s+uint64_t first_id;\s+char prefix\[32\];"
                     r"\s+uint32_t reserved\[4\];", header)
    assert "merge_reads.cpp:335-340,379-382,635-647" in header
    sig = inspect.signature(kcount.KmerCounter.fastq_text).parameters
    assert list(sig)[1:] == ["bases", "quals", "offsets", "order", "ids", "prefix", "paired", "first_id", "check", "first_byte", "capacity", "nreads"]
    assert [sig[n].default for n in list(sig)[4:]] == [None, None, "r", False, 0, False, 0, None, None]
    sig = inspect.signature(kcount.KmerCounter.write_fastq).parameters
    assert list(sig)[1:5] == ["path_or_fileobj", "bases", "quals", "offsets"] and sig["window_bytes"].default == 256 << 20
    assert (sig["order"].default, sig["ids"].default, sig["prefix"].default, sig["paired"].default, sig["check"].default) == (None, None, "r", False, False)
    sig = inspect.signature(kcount.KmerCounter.write_fastq_pairs).parameters
    assert list(sig)[1:6] == ["path1", "path2", "bases", "quals", "offsets"]
    assert (sig["first_pair"].default, sig["npairs"].default, sig["window_bytes"].default) == (0, None, 256 << 20)


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    bases = np.frombuffer(b"ACGTGGNT", dtype=np.uint8).copy()
    quals = np.full(8, ord("I"), dtype=np.uint8)
    offsets = np.array([0, 4, 7, 7, 8], dtype=np.uint64)
    order = np.full(8, 0xA5A5A5A5, dtype=np.uint32)
    text = np.full(64, 0xA5, dtype=np.uint8)
    written, total = C.c_uint64(7), C.c_uint64(7)

    def call(flags=0, nreads=4, n_order=4, order_ptr=None, q=quals, w=written, t=total, p=True, **kw):
        prm = _lib.kc_fastq_out_params(**dict(dict(flags=flags, prefix_len=1, prefix=b"r"), **kw))
        return L.kc_fastq_text(None, bases.ctypes.data, None if q is None else q.ctypes.data, offsets.ctypes.data, nreads, order_ptr, n_order, None, 0,
                               C.byref(prm) if p else None, 0, text.ctypes.data, 64, w and C.byref(w), t and C.byref(t))

    def reserved(at, value):
        r = (C.c_uint32 * 4)()
        r[at] = value
        return r

    E, CAP = _lib.KC_ERR_INVALID_ARG, _lib.KC_ERR_CAPACITY
    bad = [(lambda: call(flags=8), E, "kc_fastq_text: unknown flags 0x8"),
           (lambda: call(flags=0x80000003, q=None), E, "kc_fastq_text: unknown flags 0x80000000"),
           (lambda: call(reserved=reserved(0, 1)), E, "kc_fastq_text: reserved[0] is 1, not zero"),
           (lambda: call(reserved=reserved(3, 9)), E, "kc_fastq_text: reserved[3] is 9, not zero"),
           (lambda: call(prefix_len=33), E, "kc_fastq_text: prefix_len 33 over 32"),
           (lambda: call(prefix_len=5, prefix=b"re d_"), E, "kc_fastq_text: prefix[2] is 0x20, outside 0x21 .. 0x7e"),
           (lambda: call(prefix_len=2, prefix=b"r\x7f"), E, "kc_fastq_text: prefix[1] is 0x7f, outside 0x21 .. 0x7e"),
           (lambda: call(flags=1), E, "kc_fastq_text: KC_FASTQ_OUT_PACKED and quals is not NULL"),
           (lambda: call(flags=2, q=None), E, "kc_fastq_text: quals is NULL for 4 reads without KC_FASTQ_OUT_PACKED"),
           (lambda: call(p=False), E, "kc_fastq_text: params is NULL"),
           (lambda: call(w=None), E, "kc_fastq_text: written is NULL"),
           (lambda: call(t=None), E, "kc_fastq_text: total is NULL"),
           (lambda: call(n_order=3), E, "kc_fastq_text: order is NULL and n_order 3 is not the 4 reads"),
           (lambda: call(nreads=1 << 32, n_order=1 << 32), CAP, "kc_fastq_text: 4294967296 reads and 4294967296 records, read and record indices"),
           (lambda: call(n_order=1 << 32, order_ptr=order.ctypes.data), CAP, "kc_fastq_text: 4 reads and 4294967296 records, read and record indices")]
    for f, status, message in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)  # leaves another text behind
        assert f() == status, message
        assert message.encode() in L.kc_last_error(), (message, L.kc_last_error())
    # in range, the corners included, the calls get as far as the NULL context and leave the text alone
    marker = L.kc_last_error()
    good = [lambda: call(), lambda: call(flags=7, q=None), lambda: call(flags=6), lambda: call(prefix_len=0, prefix=b""),
            lambda: call(prefix_len=32, prefix=b"!" * 31 + b"~", first_id=(1 << 64) - 1), lambda: call(n_order=2, order_ptr=order.ctypes.data),
            lambda: call(nreads=0, n_order=0, q=None), lambda: call(nreads=(1 << 32) - 1, n_order=(1 << 32) - 1),
            lambda: call(prefix_len=1, prefix=b"r x")]  # bytes behind prefix_len are not read
    for f in good:
        assert f() == E
        assert L.kc_last_error() == marker
    assert (written.value, total.value) == (7, 7)
    assert (order == 0xA5A5A5A5).all() and (text == 0xA5).all()
