"""kc_ctg_break is exported, its parameters, pieces, records and statistics have the layout the fourth header states, the Python
defaults are the model's, and every range that needs no device is refused in front of the context, by the values
kc_last_error names, with nothing written through any pointer (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import break_cases as BC
import break_model as M
import mhm2_kmer_analysis_v2_amd as pkg
import test_kdepth_abi as A
from mhm2_kmer_analysis_v2_amd import _lib, kcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kcount_mi355_break.h")).read()
KERNELS = open(os.path.join(ROOT, "mhm2_kmer_analysis_v2_amd", "csrc", "kc_break.hpp")).read()


def header_layout(name):
    """test_kdepth_abi's parse, over the fourth header"""
    first, A.HEADER = A.HEADER, HEADER
    try:
        return A.header_layout(name)
    finally:
        A.HEADER = first


def test_symbol_is_exported_and_bound_from_the_fourth_table():
    L = pkg.lib()
    assert L.kc_ctg_break.restype is C.c_int and len(L.kc_ctg_break.argtypes) == 21
    assert "kc_ctg_break" in _lib.SYMBOLS_BREAK
    assert not any("kc_ctg_break" in t for t in (_lib.SYMBOLS, _lib.SYMBOLS_CORRECT, _lib.SYMBOLS_POLISH))
    assert callable(kcount.KmerCounter.break_contigs) and callable(kcount.KmerCounter.break_strings) and callable(pkg.break_strings)
    assert L.kc_abi_version() == 1
    assert pkg.BREAK_DTYPE is kcount.BREAK_DTYPE and pkg.BREAK_PIECE_DTYPE is kcount.BREAK_PIECE_DTYPE


def test_layouts_constants_and_defaults():
    for name, size in (("kc_break_params", 32), ("kc_break_piece", 16), ("kc_break_rec", 32), ("kc_break_stats", 128)):
        struct = getattr(_lib, name)
        fields, total = header_layout(name)
        assert total == size == C.sizeof(struct), name
        assert fields == [(n, getattr(struct, n).offset) for n, _ in struct._fields_], name
    piece = [("ctg", 0), ("start", 4), ("len", 8), ("flags", 12)]
    rec = [("ctg", 0), ("pos", 4), ("run_start", 8), ("run_len", 12), ("span", 16), ("disc", 20), ("piece", 24), ("pad", 28)]
    for dtype in (M.PIECE_DTYPE, kcount.BREAK_PIECE_DTYPE):
        assert dtype.itemsize == 16 and [(n, dtype.fields[n][1]) for n in dtype.names] == piece
    for dtype in (M.BREAK_DTYPE, kcount.BREAK_DTYPE):
        assert dtype.itemsize == 32 and [(n, dtype.fields[n][1]) for n in dtype.names] == rec
    assert header_layout("kc_break_piece")[0] == piece and header_layout("kc_break_rec")[0] == rec
    assert [n for n, _ in _lib.kc_break_stats._fields_ if n != "reserved"] == list(M.STATS)
    assert _lib.KC_BREAK_ONE_MATE == M.ONE_MATE == 1 and re.search(r"#define KC_BREAK_ONE_MATE 1u\b", HEADER)
    assert M.INSERT_MAX == _lib.KC_INSERT_MAX and M.NO_ALN == 0xFFFFFFFF
    assert BC.GAP_ALN_DTYPE == kcount.GAP_ALN_DTYPE and BC.PAIR_DTYPE == kcount.PAIR_DTYPE
    # the scan tile T is named in the header's text and is the kernels'
    assert re.search(r"constexpr uint32_t BREAK_TILE = BREAK_TPB \* BREAK_ITEMS;", KERNELS) and re.search(r"constexpr int BREAK_TPB = 256;", KERNELS)
    assert re.search(r"constexpr int BREAK_ITEMS = 8;", KERNELS) and BC.T == 256 * 8 and re.search(r"tiles of T = %d columns" % BC.T, HEADER)
    sig = inspect.signature(kcount.KmerCounter.break_contigs).parameters
    assert list(sig)[1:] == ["offsets", "gap_alns", "pairs", "depths", "max_insert", "max_span", "min_disc", "margin", "min_run", "one_mate", "tracks"]
    assert sig["depths"].default is None and sig["tracks"].default is False
    model = inspect.signature(M.break_contigs).parameters
    for n, v in M.DEFAULTS.items():
        assert model[n].default == sig[n].default == v, n


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    offsets = np.zeros(5, dtype=np.uint64)
    outs = [np.full(64, 0xA5, dtype=np.uint8) for _ in range(7)]
    st = _lib.kc_break_stats(pairs=7, breaks=7)
    n_out, nbytes_out = C.c_uint64(0xA5), C.c_uint64(0xA5)

    def brk(params=True, nreads=4, n_out_p=True, nbytes_out_p=True, reserved=(0, 0), **kw):
        p = _lib.kc_break_params(**dict(dict(max_insert=1000, max_span=0, min_disc=3, margin=1000, min_run=1, flags=0), **kw))
        p.reserved[0], p.reserved[1] = reserved
        o = [a.ctypes.data for a in outs]
        return L.kc_ctg_break(None, offsets.ctypes.data, nreads, None, 0, None, None, 0, C.byref(p) if params else None, o[0], 64, o[1], o[2], o[3], o[4], 2,
                              o[5], o[6], C.byref(n_out) if n_out_p else None, C.byref(nbytes_out) if nbytes_out_p else None, C.byref(st))

    bad = [(lambda: brk(params=False), "kc_ctg_break: params is NULL"),
           (lambda: brk(n_out_p=False), "kc_ctg_break: n_out is NULL"),
           (lambda: brk(nbytes_out_p=False), "kc_ctg_break: nbytes_out is NULL"),
           (lambda: brk(flags=2), "kc_ctg_break: unknown flags 0x2"),
           (lambda: brk(flags=0x80000001), "kc_ctg_break: unknown flags 0x80000000"),
           (lambda: brk(reserved=(0, 9)), "kc_ctg_break: reserved[1] is 9, not zero"),
           (lambda: brk(reserved=(3, 0)), "kc_ctg_break: reserved[0] is 3, not zero"),
           (lambda: brk(max_insert=0), "kc_ctg_break: max_insert 0 outside 1 .. 65535"),
           (lambda: brk(max_insert=65536), "kc_ctg_break: max_insert 65536 outside 1 .. 65535"),
           (lambda: brk(margin=0), "kc_ctg_break: margin is 0, at least 1"),
           (lambda: brk(min_run=0), "kc_ctg_break: min_run is 0, at least 1"),
           (lambda: brk(nreads=3), "kc_ctg_break: 3 reads are no pairs"),
           (lambda: brk(), "kc_ctg_break: ctx is NULL"),
           (lambda: brk(max_insert=65535, max_span=0xFFFFFFFF, min_disc=0, margin=0xFFFFFFFF, min_run=0xFFFFFFFF, flags=1), "kc_ctg_break: ctx is NULL"),
           (lambda: brk(max_insert=1, margin=1, min_run=1, min_disc=0xFFFFFFFF), "kc_ctg_break: ctx is NULL")]  # in range
    for call, message in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)  # leaves another text behind
        assert call() == _lib.KC_ERR_INVALID_ARG, message
        assert message.encode() in L.kc_last_error(), (message, L.kc_last_error())
    assert (st.pairs, st.breaks, st.weak) == (7, 7, 0) and (n_out.value, nbytes_out.value) == (0xA5, 0xA5)
    assert all((a == 0xA5).all() for a in outs)
