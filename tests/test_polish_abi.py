"""kc_ctg_polish is exported, its parameters, records, fixes and statistics have the layout the third header states, the Python
defaults are the model's, and every range that needs no device is refused in front of the context, by the values
kc_last_error names, with nothing written through any pointer (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import polish_cases as PC
import polish_model as M
import mhm2_kmer_analysis_v2_amd as pkg
import test_kdepth_abi as A
from mhm2_kmer_analysis_v2_amd import _lib, kcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kcount_mi355_polish.h")).read()
KERNELS = open(os.path.join(ROOT, "mhm2_kmer_analysis_v2_amd", "csrc", "kc_polish.hpp")).read()


def header_layout(name):
    """test_kdepth_abi's parse, over the third header"""
    first, A.HEADER = A.HEADER, HEADER
    try:
        return A.header_layout(name)
    finally:
        A.HEADER = first


def test_symbol_is_exported_and_bound_from_the_third_table():
    L = pkg.lib()
    assert L.kc_ctg_polish.restype is C.c_int and len(L.kc_ctg_polish.argtypes) == 15
    assert "kc_ctg_polish" in _lib.SYMBOLS_POLISH and "kc_ctg_polish" not in _lib.SYMBOLS and "kc_ctg_polish" not in _lib.SYMBOLS_CORRECT
    assert callable(kcount.KmerCounter.polish_contigs) and callable(pkg.polish_strings) and L.kc_abi_version() == 1
    assert pkg.POLISH_CTG_DTYPE is kcount.POLISH_CTG_DTYPE and pkg.POLISH_FIX_DTYPE is kcount.POLISH_FIX_DTYPE


def test_layouts_constants_and_defaults():
    for name, size in (("kc_polish_params", 32), ("kc_polish_ctg", 32), ("kc_polish_fix", 16), ("kc_polish_stats", 128)):
        struct = getattr(_lib, name)
        fields, total = header_layout(name)
        assert total == size == C.sizeof(struct), name
        assert fields == [(n, getattr(struct, n).offset) for n, _ in struct._fields_], name
    ctg = [("votes", 0), ("placed", 8), ("changed", 12), ("filled", 16), ("disputed", 20), ("thin", 24), ("uncovered", 28)]
    fix = [("pos", 0), ("ctg", 4), ("old", 8), ("new", 9), ("top", 10), ("tot", 12), ("pad", 14)]
    for dtype in (M.CTG_DTYPE, kcount.POLISH_CTG_DTYPE):
        assert dtype.itemsize == 32 and [(n, dtype.fields[n][1]) for n in dtype.names] == ctg
    for dtype in (M.FIX_DTYPE, kcount.POLISH_FIX_DTYPE):
        assert dtype.itemsize == 16 and [(n, dtype.fields[n][1]) for n in dtype.names] == fix
    assert header_layout("kc_polish_ctg")[0] == ctg
    assert [at for _, at in header_layout("kc_polish_fix")[0]] == [at for _, at in fix]
    assert [n for n, _ in _lib.kc_polish_stats._fields_] == list(M.STATS)
    assert _lib.KC_POLISH_BEST_ONLY == M.BEST_ONLY == 1 and re.search(r"#define KC_POLISH_BEST_ONLY 1u\b", HEADER)
    assert M.MAX_EDGE == _lib.KC_DEPTH_MAX_EDGE and re.search(r"POLISH_MAX_PERMILLE = %d, POLISH_MAX_QUAL = %d;" % (M.MAX_PERMILLE, M.MAX_QUAL), KERNELS)
    assert re.search(r"constexpr uint32_t POLISH_TILE = %d;" % PC.TILE, KERNELS)
    sig = inspect.signature(kcount.KmerCounter.polish_contigs).parameters
    assert list(sig)[1:] == ["bases", "offsets", "gap_alns", "quals", "min_score", "min_len", "edge_clip", "max_mismatches", "min_depth",
                             "min_permille", "min_qual", "best_only", "with_counts", "with_records", "with_fixes"]
    assert [sig[n].default for n in ("quals", "with_counts", "with_records", "with_fixes")] == [None, False, True, True]
    model = inspect.signature(M.polish).parameters
    for n, v in M.DEFAULTS.items():
        assert model[n].default == sig[n].default == v, n


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    c = PC.case("empty")
    bases, offsets, _ = c.block()
    out = np.full(200, 0xA5, dtype=np.uint8)
    counts = np.full(200 * 4, 0xA5A5, dtype=np.uint16)
    ctgs = np.full(2 * 32, 0xA5, dtype=np.uint8)
    fixes = np.full(4 * 16, 0xA5, dtype=np.uint8)
    st = _lib.kc_polish_stats(records=7, changed=7)

    def polish(params=True, **kw):
        p = _lib.kc_polish_params(**dict(dict(max_mismatches=8, min_depth=3, min_permille=700), **kw))
        return L.kc_ctg_polish(None, bases.ctypes.data, None, offsets.ctypes.data, 1, None, 0, 0, C.byref(p) if params else None, out.ctypes.data,
                               counts.ctypes.data, ctgs.ctypes.data, fixes.ctypes.data, 4, C.byref(st))

    bad = [(lambda: polish(params=False), "kc_ctg_polish: params is NULL"),
           (lambda: polish(flags=2), "kc_ctg_polish: edge_clip 0 over 1024 or unknown flags 0x2"),
           (lambda: polish(edge_clip=1025), "kc_ctg_polish: edge_clip 1025 over 1024 or unknown flags 0x0"),
           (lambda: polish(min_depth=0), "kc_ctg_polish: min_depth is 0, at least 1"),
           (lambda: polish(min_permille=1001), "kc_ctg_polish: min_permille is 1001, at most 1000"),
           (lambda: polish(min_qual=256), "kc_ctg_polish: min_qual is 256, at most 255"),
           (lambda: polish(), "kc_ctg_polish: ctx is NULL"),
           (lambda: polish(edge_clip=1024, min_permille=1000, min_qual=255, flags=1, max_mismatches=0xFFFFFFFF, min_depth=0xFFFFFFFF),
            "kc_ctg_polish: ctx is NULL")]  # in range
    for call, message in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)  # leaves another text behind
        assert call() == _lib.KC_ERR_INVALID_ARG, message
        assert message.encode() in L.kc_last_error(), (message, L.kc_last_error())
    assert (st.records, st.changed, st.placed) == (7, 7, 0)
    assert (out == 0xA5).all() and (counts == 0xA5A5).all() and (ctgs == 0xA5).all() and (fixes == 0xA5).all()
