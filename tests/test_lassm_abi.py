"""kc_local_assm is exported, its parameters, records and statistics have the layout the header states, and every range
that needs no device is refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import lassm_model as M

GOOD = dict(min_mer_len=13, max_mer_len=121, shift=8, max_walk_len=400, max_insert=1000, min_qual=10, hi_qual=20, min_viable=2,
            viable_permille=200, max_cands=2000, table_budget_mb=0, flags=0)


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_local_assm" in _lib.SYMBOLS
    f = L.kc_local_assm
    assert f.restype is C.c_int and len(f.argtypes) == 17
    assert callable(kcount.KmerCounter.local_assm)
    assert L.kc_abi_version() == 1


def test_layouts():
    assert (C.sizeof(_lib.kc_lassm_params), C.sizeof(_lib.kc_lassm_end), C.sizeof(_lib.kc_lassm_stats)) == (48, 16, 144)
    assert [n for n, _ in _lib.kc_lassm_params._fields_] == list(GOOD) == list(M.DEFAULTS)
    assert [getattr(_lib.kc_lassm_params, n).offset for n in GOOD] == list(range(0, 48, 4))
    assert [(n, getattr(_lib.kc_lassm_end, n).offset) for n, _ in _lib.kc_lassm_end._fields_] == [
        ("cands", 0), ("ext_len", 4), ("out_pos", 8), ("iters", 12), ("mer_len", 14), ("status", 15)]
    for dt in (kcount.LASSM_END_DTYPE, M.LASSM_END_DTYPE):
        assert dt.itemsize == 16
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(_lib.kc_lassm_end, n).offset) for n, _ in _lib.kc_lassm_end._fields_]
    assert [(n, getattr(_lib.kc_lassm_stats, n).offset) for n, _ in _lib.kc_lassm_stats._fields_] == [
        ("ends", 0), ("status", 8), ("cands_overhang", 56), ("cands_mate", 64), ("cand_bases", 72), ("iterations", 80), ("ext_bases", 88),
        ("ctgs_extended", 96), ("reserved", 104)]
    assert [n for n, _ in _lib.kc_lassm_stats._fields_][:-1] == list(M.LASSM_STATS)
    assert (_lib.KC_LASSM_MAX_MER_LEN, _lib.KC_LASSM_MAX_WALK, _lib.KC_LASSM_MAX_CANDS) == (M.MAX_MER_LEN, M.MAX_WALK, M.MAX_CANDS) == (
        128, 4096, 1 << 20)
    assert (_lib.KC_LASSM_NO_CANDS, _lib.KC_LASSM_TOO_MANY, _lib.KC_LASSM_DEAD_END, _lib.KC_LASSM_FORK, _lib.KC_LASSM_LOOP,
            _lib.KC_LASSM_MAX_LEN) == (M.NO_CANDS, M.TOO_MANY, M.DEAD_END, M.FORK, M.LOOP, M.MAX_LEN) == tuple(range(6))
    import inspect
    sig = inspect.signature(kcount.KmerCounter.local_assm).parameters
    assert {n: sig[n].default for n in GOOD if n not in ("table_budget_mb", "flags")} == {
        n: v for n, v in M.DEFAULTS.items() if n not in ("table_budget_mb", "flags")}


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    offs = np.zeros(4, dtype=np.uint64)
    alns = np.zeros(1, dtype=kcount.GAP_ALN_DTYPE)
    pairs = np.zeros(1, dtype=kcount.PAIR_DTYPE)
    seqs = np.full(64, 0xAB, dtype=np.uint8)
    offs_out = np.full(4, 0xABAB, dtype=np.uint64)
    ends = np.full(64, 0xAB, dtype=np.uint8)
    nb = C.c_uint64(7)
    st = _lib.kc_lassm_stats(ends=7, ctgs_extended=7)

    def call(nreads=2, **kw):
        p = _lib.kc_lassm_params(**dict(GOOD, **kw))
        return L.kc_local_assm(None, None, None, offs.ctypes.data, nreads, alns.ctypes.data, 1, pairs.ctypes.data, None, 0, C.byref(p),
                               seqs.ctypes.data, 64, offs_out.ctypes.data, ends.ctypes.data, C.byref(nb), C.byref(st))

    bad = [
        (dict(min_mer_len=3), b"kc_local_assm: mer lengths 3 .. 121 by 8 outside"),
        (dict(min_mer_len=122), b"kc_local_assm: mer lengths 122 .. 121 by 8 outside"),
        (dict(max_mer_len=129), b"kc_local_assm: mer lengths 13 .. 129 by 8 outside"),
        (dict(shift=0), b"kc_local_assm: mer lengths 13 .. 121 by 0 outside"),
        (dict(shift=65), b"kc_local_assm: mer lengths 13 .. 121 by 65 outside"),
        (dict(max_walk_len=0), b"kc_local_assm: max_walk_len 0 outside 1 .. 4096"),
        (dict(max_walk_len=4097), b"kc_local_assm: max_walk_len 4097 outside 1 .. 4096"),
        (dict(max_insert=0), b"kc_local_assm: max_insert 0 outside 1 .. 65535"),
        (dict(max_insert=65536), b"kc_local_assm: max_insert 65536 outside 1 .. 65535"),
        (dict(min_qual=21), b"kc_local_assm: qualities 21 20 outside min_qual <= hi_qual <= 93"),
        (dict(hi_qual=94), b"kc_local_assm: qualities 10 94 outside min_qual <= hi_qual <= 93"),
        (dict(min_viable=0), b"kc_local_assm: min_viable 0 under 1 or viable_permille 200 over 1000"),
        (dict(viable_permille=1001), b"kc_local_assm: min_viable 2 under 1 or viable_permille 1001 over 1000"),
        (dict(max_cands=0), b"kc_local_assm: max_cands 0 outside 1 .. 1048576"),
        (dict(max_cands=(1 << 20) + 1), b"kc_local_assm: max_cands 1048577 outside 1 .. 1048576"),
        (dict(flags=1), b"kc_local_assm: unknown flags 0x1"),
        (dict(flags=0x80000000), b"kc_local_assm: unknown flags 0x80000000"),
    ]
    for kw, text in bad:
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert text in L.kc_last_error(), (kw, L.kc_last_error())
    assert call(nreads=3) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_local_assm: 3 reads are no pairs" in L.kc_last_error()
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    for kw in (dict(min_mer_len=4, max_mer_len=4, shift=1), dict(min_mer_len=128, max_mer_len=128, shift=64), dict(max_walk_len=1),
               dict(max_walk_len=4096), dict(max_insert=1), dict(max_insert=65535), dict(min_qual=0, hi_qual=0), dict(min_qual=93, hi_qual=93),
               dict(min_viable=1, viable_permille=0), dict(min_viable=0xFFFFFFFF, viable_permille=1000), dict(max_cands=1),
               dict(max_cands=1 << 20), dict(table_budget_mb=0xFFFFFFFF)):
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert b"3 reads are no pairs" in L.kc_last_error(), kw
    assert (nb.value, st.ends, st.ctgs_extended) == (7, 7, 7)
    assert (seqs == 0xAB).all() and (offs_out == 0xABAB).all() and (ends == 0xAB).all()
