"""kc_shuffle_reads is exported, its statistics have the layout the header states, and every argument error that needs no
device is refused in front of the context, by the values kc_last_error names, with nothing written (no GPU needed)."""
import ctypes as C
import inspect

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import shuffle_model as M


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_shuffle_reads" in _lib.SYMBOLS
    f = L.kc_shuffle_reads
    assert f.restype is C.c_int and len(f.argtypes) == 19
    assert callable(kcount.KmerCounter.shuffle_reads)
    sig = inspect.signature(kcount.KmerCounter.shuffle_reads).parameters
    assert list(sig) == ["self", "bases", "quals", "offsets", "gap_alns", "pairs", "parts", "remap"]
    assert (sig["parts"].default, sig["remap"].default) == (1, True)
    assert L.kc_abi_version() == 1


def test_layouts():
    assert C.sizeof(_lib.kc_shuffle_stats) == 80
    assert [n for n, _ in _lib.kc_shuffle_stats._fields_] == list(M.SHUFFLE_STATS)
    assert [getattr(_lib.kc_shuffle_stats, n).offset for n in M.SHUFFLE_STATS] == list(range(0, 80, 8))
    assert (_lib.KC_SHUFFLE_MAX_PARTS, _lib.KC_SHUFFLE_NO_HOME) == (M.MAX_PARTS, M.NO_HOME) == (65536, 0xFFFFFFFF)


def test_argument_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    n = 4  # reads
    ins = {"bases": np.full(64, ord("A"), dtype=np.uint8), "quals": np.full(64, ord("I"), dtype=np.uint8),
           "offsets": np.arange(n + 1, dtype=np.uint64) * 16, "alns": np.zeros(1, dtype=kcount.GAP_ALN_DTYPE),
           "pairs": np.zeros(n // 2, dtype=kcount.PAIR_DTYPE)}
    outs = {"bases_out": np.full(64, 0xAB, dtype=np.uint8), "quals_out": np.full(64, 0xAB, dtype=np.uint8),
            "offsets_out": np.full(n + 1, 0xABAB, dtype=np.uint64), "order": np.full(n // 2, 0xABAB, dtype=np.uint32),
            "home": np.full(n // 2, 0xABAB, dtype=np.uint32), "part_starts": np.full(9, 0xABAB, dtype=np.uint64),
            "alns_out": np.full(32, 0xAB, dtype=np.uint8), "pairs_out": np.full(32, 0xAB, dtype=np.uint8)}
    images = {k: v.tobytes() for k, v in list(ins.items()) + list(outs.items())}
    st = _lib.kc_shuffle_stats(pairs=7, key_bits=7)

    def call(nreads=n, parts=1, **kw):
        """kw: an argument's name -> None, or the name of the array to pass in its place"""
        a = {k: v.ctypes.data for k, v in list(ins.items()) + list(outs.items())}
        for k, v in kw.items():
            a[k] = None if v is None else a[v]
        return L.kc_shuffle_reads(None, a["bases"], a["quals"], a["offsets"], nreads, a["alns"], 1, a["pairs"], 0, parts, a["bases_out"],
                                  a["quals_out"], a["offsets_out"], a["order"], a["home"], a["part_starts"], a["alns_out"], a["pairs_out"],
                                  C.byref(st))

    bad = [(dict(nreads=3), b"kc_shuffle_reads: 3 reads are no pairs"),
           (dict(nreads=1), b"kc_shuffle_reads: 1 reads are no pairs"),
           (dict(parts=0), b"kc_shuffle_reads: parts 0 outside 1 .. 65536"),
           (dict(parts=65537), b"kc_shuffle_reads: parts 65537 outside 1 .. 65536"),
           (dict(parts=0xFFFFFFFF), b"kc_shuffle_reads: parts 4294967295 outside 1 .. 65536"),
           (dict(pairs=None), b"kc_shuffle_reads: pairs is NULL"),
           (dict(quals=None), b"kc_shuffle_reads: quals is NULL and quals_out is given"),
           (dict(quals_out=None), b"kc_shuffle_reads: quals is given and quals_out is NULL")]
    bad += [({k: None}, b"kc_shuffle_reads: %s is NULL" % k.encode()) for k in ("bases_out", "offsets_out", "order", "home", "part_starts")]
    bad += [({o: i}, b"kc_shuffle_reads: %s is %s" % (o.encode(), i.encode()))
            for o, i in (("bases_out", "bases"), ("quals_out", "quals"), ("bases_out", "quals"), ("offsets_out", "offsets"), ("alns_out", "alns"),
                         ("pairs_out", "pairs"), ("order", "pairs"), ("home", "offsets"), ("part_starts", "offsets"), ("quals_out", "bases"))]
    for kw, text in bad:
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert text in L.kc_last_error(), (kw, L.kc_last_error())
    # the first of two errors is the one named: the reads, then the parts, then the pointers
    assert call(nreads=3, parts=0, order=None) == _lib.KC_ERR_INVALID_ARG and b"3 reads are no pairs" in L.kc_last_error()
    assert call(parts=0, order=None) == _lib.KC_ERR_INVALID_ARG and b"parts 0 outside" in L.kc_last_error()
    # the model refuses the same values
    for kw in (dict(nreads=3), dict(parts=0), dict(parts=65537)):
        try:
            M.shuffle_reads([10], b"", None, np.zeros(kw.get("nreads", 0) + 1, dtype=np.uint64), ins["alns"][:0], ins["pairs"][:0], kw.get("parts", 1))
        except M.BadArg as e:
            assert call(**kw) == _lib.KC_ERR_INVALID_ARG and str(e).encode() in L.kc_last_error(), (str(e), L.kc_last_error())
        else:
            raise AssertionError("the model took %r" % (kw,))
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    assert call(nreads=3) == _lib.KC_ERR_INVALID_ARG
    for kw in (dict(parts=1), dict(parts=65536), dict(alns_out=None), dict(pairs_out=None), dict(alns_out=None, pairs_out=None),
               dict(quals=None, quals_out=None), dict(nreads=0, pairs=None)):
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert b"3 reads are no pairs" in L.kc_last_error(), kw
    assert (st.pairs, st.key_bits, st.homed) == (7, 7, 0)
    for k, v in list(ins.items()) + list(outs.items()):
        assert v.tobytes() == images[k], k
