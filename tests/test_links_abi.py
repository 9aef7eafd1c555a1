"""kc_ctg_links is exported, its parameters, records and statistics have the layout the header states, and every range
that needs no device is refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import links_model as M

GOOD = dict(min_score=0, min_len=0, end_slack=5, max_overlap=200, max_splint_gap=100, insert_avg=300, max_insert=1000, max_read_alns=8, flags=0)


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_ctg_links" in _lib.SYMBOLS
    f = L.kc_ctg_links
    assert f.restype is C.c_int and len(f.argtypes) == 13
    assert callable(kcount.KmerCounter.ctg_links)
    assert L.kc_abi_version() == 1


def test_layouts():
    assert (C.sizeof(_lib.kc_link_params), C.sizeof(_lib.kc_ctg_link), C.sizeof(_lib.kc_link_stats)) == (32, 48, 128)
    assert [n for n, _ in _lib.kc_link_params._fields_] == list(GOOD) == list(M.DEFAULTS) and GOOD == M.DEFAULTS
    assert [getattr(_lib.kc_link_params, n).offset for n in GOOD] == [0, 4, 8, 12, 16, 20, 24, 28, 30]
    want = [("from", 0), ("to", 4), ("splints", 8), ("spans", 12), ("splint_gap_min", 16), ("splint_gap_max", 20), ("span_gap_min", 24),
            ("span_gap_max", 28), ("splint_gap_sum", 32), ("span_gap_sum", 40)]
    assert [(n.rstrip("_"), getattr(_lib.kc_ctg_link, n).offset) for n, _ in _lib.kc_ctg_link._fields_] == want
    for dt in (kcount.LINK_DTYPE, M.LINK_DTYPE):
        assert dt.itemsize == 48 and [(n, dt.fields[n][1]) for n in dt.names] == want
        assert [dt.fields[n][0].kind for n in dt.names] == ["u"] * 4 + ["i"] * 6
    assert [n for n, _ in _lib.kc_link_stats._fields_] == list(M.LINK_STATS) + ["reserved"]
    assert [getattr(_lib.kc_link_stats, n).offset for n, _ in _lib.kc_link_stats._fields_] == list(range(0, 128, 8))
    assert (_lib.KC_LINK_MAX_SLACK, _lib.KC_LINK_MAX_OVERLAP, _lib.KC_LINK_MAX_READ_ALNS) == (M.MAX_SLACK, M.MAX_OVERLAP, M.MAX_READ_ALNS) == (
        1024, 65535, 64)
    sig = inspect.signature(kcount.KmerCounter.ctg_links).parameters
    assert {n: sig[n].default for n in GOOD if n != "flags"} == {n: v for n, v in M.DEFAULTS.items() if n != "flags"}


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    offs = np.zeros(4, dtype=np.uint64)
    alns = np.zeros(1, dtype=kcount.GAP_ALN_DTYPE)
    pairs = np.zeros(1, dtype=kcount.PAIR_DTYPE)
    links = np.full(96, 0xAB, dtype=np.uint8)
    end_first = np.full(4, 0xABAB, dtype=np.uint64)
    n = C.c_uint64(7)
    st = _lib.kc_link_stats(reads=7, ends_linked=7)

    def call(nreads=2, **kw):
        p = _lib.kc_link_params(**dict(GOOD, **kw))
        return L.kc_ctg_links(None, offs.ctypes.data, nreads, alns.ctypes.data, 1, pairs.ctypes.data, 0, C.byref(p), links.ctypes.data, 2,
                              end_first.ctypes.data, C.byref(n), C.byref(st))

    bad = [
        (dict(end_slack=1025), b"kc_ctg_links: end_slack 1025 over 1024"),
        (dict(end_slack=0xFFFFFFFF), b"kc_ctg_links: end_slack 4294967295 over 1024"),
        (dict(max_overlap=65536), b"kc_ctg_links: max_overlap 65536 over 65535 or max_splint_gap 100 over 1024"),
        (dict(max_splint_gap=1025), b"kc_ctg_links: max_overlap 200 over 65535 or max_splint_gap 1025 over 1024"),
        (dict(insert_avg=0), b"kc_ctg_links: insert_avg 0, max_insert 1000 outside 1 <= insert_avg <= max_insert <= 65535"),
        (dict(insert_avg=1001), b"kc_ctg_links: insert_avg 1001, max_insert 1000 outside"),
        (dict(max_insert=299), b"kc_ctg_links: insert_avg 300, max_insert 299 outside"),
        (dict(max_insert=65536), b"kc_ctg_links: insert_avg 300, max_insert 65536 outside"),
        (dict(max_read_alns=1), b"kc_ctg_links: max_read_alns 1 outside 2 .. 64"),
        (dict(max_read_alns=0), b"kc_ctg_links: max_read_alns 0 outside 2 .. 64"),
        (dict(max_read_alns=65), b"kc_ctg_links: max_read_alns 65 outside 2 .. 64"),
        (dict(flags=1), b"kc_ctg_links: unknown flags 0x1"),
        (dict(flags=0x8000), b"kc_ctg_links: unknown flags 0x8000"),
    ]
    for kw, text in bad:
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert text in L.kc_last_error(), (kw, L.kc_last_error())
        try:
            M.ctg_links([10], [0, 0], np.zeros(0, dtype=M.GAP_ALN_DTYPE), **kw)
        except M.BadArg as e:
            assert str(e).encode() in L.kc_last_error(), (str(e), L.kc_last_error())  # the model names the same values
        else:
            raise AssertionError("the model took %r" % (kw,))
    assert call(nreads=3) == _lib.KC_ERR_INVALID_ARG
    assert b"kc_ctg_links: 3 reads are no pairs" in L.kc_last_error()
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    for kw in (dict(end_slack=0), dict(end_slack=1024), dict(max_overlap=0), dict(max_overlap=65535), dict(max_splint_gap=0),
               dict(max_splint_gap=1024), dict(insert_avg=1, max_insert=1), dict(insert_avg=65535, max_insert=65535), dict(insert_avg=1, max_insert=65535),
               dict(max_read_alns=2), dict(max_read_alns=64), dict(min_score=0xFFFFFFFF, min_len=0xFFFFFFFF)):
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert b"3 reads are no pairs" in L.kc_last_error(), kw
    # the parameters and the count are required
    assert L.kc_ctg_links(None, None, 0, None, 0, None, 0, None, None, 0, None, C.byref(n), None) == _lib.KC_ERR_INVALID_ARG
    p = _lib.kc_link_params(**GOOD)
    assert L.kc_ctg_links(None, None, 0, None, 0, None, 0, C.byref(p), None, 0, None, None, None) == _lib.KC_ERR_INVALID_ARG
    assert (n.value, st.reads, st.ends_linked) == (7, 7, 7)
    assert (links == 0xAB).all() and (end_first == 0xABAB).all()
