"""kc_close_gaps is exported, its parameters, records and statistics have the layout the header states, and every range that
needs no device is refused in front of the context, by the values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect

import numpy as np

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

import close_cases as CC
import close_model as M
from test_close_model import BAD_PARAMS, GOOD_PARAMS

GOOD = dict(M.DEFAULTS)


def test_symbol_is_exported():
    L = pkg.lib()
    assert "kc_close_gaps" in _lib.SYMBOLS
    f = L.kc_close_gaps
    assert f.restype is C.c_int and len(f.argtypes) == 19
    assert callable(kcount.KmerCounter.close_gaps) and callable(kcount.KmerCounter.close_gaps_strings)
    assert L.kc_abi_version() == 1


def test_layouts():
    sizes = (C.sizeof(_lib.kc_close_params), C.sizeof(_lib.kc_closure), C.sizeof(_lib.kc_close_stats))
    assert sizes == (32, 32, 128)
    assert [n for n, _ in _lib.kc_close_params._fields_] == list(GOOD)
    assert [getattr(_lib.kc_close_params, n).offset for n, _ in _lib.kc_close_params._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 30]
    want = [("cands", 0), ("reads", 4), ("old_join", 8), ("new_join", 12), ("fill_pos", 16), ("disputed", 20), ("status", 24), ("pad", 25),
            ("reserved", 28)]
    assert [(n, getattr(_lib.kc_closure, n).offset) for n, _ in _lib.kc_closure._fields_] == want
    for dt in (kcount.CLOSURE_DTYPE, M.CLOSURE_DTYPE):
        assert dt.itemsize == 32 and [(n, dt.fields[n][1]) for n in dt.names] == want
        assert dt.fields["old_join"][0].kind == dt.fields["new_join"][0].kind == "i"
    assert [n for n, _ in _lib.kc_close_stats._fields_] == list(M.CLOSE_STATS)
    assert [getattr(_lib.kc_close_stats, n).offset for n in M.CLOSE_STATS] == list(range(0, 128, 8))
    names = ("HEAD", "NOT_A_GAP", "NO_READS", "WEAK", "FILLED", "ABUT", "OVERLAP", "OVERLAP_REJECTED")
    assert [getattr(_lib, "KC_CLOSE_" + n) for n in names] == [getattr(M, n) for n in names] == list(range(8))
    sig = inspect.signature(kcount.KmerCounter.close_gaps).parameters
    assert {n: sig[n].default for n in GOOD if n != "flags"} == {n: v for n, v in M.DEFAULTS.items() if n != "flags"}
    assert list(sig)[1:6] == ["bases", "offsets", "gap_alns", "scaffolds", "members"]


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    case = CC.two_contigs(7)
    bases = np.frombuffer("".join(case.reads).encode(), dtype=np.uint8).copy()
    roffs = np.zeros(len(case.reads) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in case.reads])
    seqs = np.full(256, 0xAB, dtype=np.uint8)
    offs = np.full(4, 0xABAB, dtype=np.uint64)
    scafs, members, closures = (np.full(64, 0xAB, dtype=np.uint8) for _ in range(3))
    nb = C.c_uint64(7)
    st = _lib.kc_close_stats(members=7, disputed_cols=7)

    def call(**kw):
        p = _lib.kc_close_params(**dict(GOOD, **kw))
        return L.kc_close_gaps(None, bases.ctypes.data, roffs.ctypes.data, len(case.reads), case.alns.ctypes.data, len(case.alns),
                               case.scaffolds.ctypes.data, 1, case.members.ctypes.data, 0, C.byref(p), seqs.ctypes.data, 256, offs.ctypes.data,
                               scafs.ctypes.data, members.ctypes.data, closures.ctypes.data, C.byref(nb), C.byref(st))

    bad = BAD_PARAMS + [(dict(end_slack=0xFFFFFFFF), "kc_close_gaps: end_slack 4294967295 over 1024"),
                        (dict(min_agree_permille=0xFFFFFFFF), "kc_close_gaps: min_agree_permille 4294967295 over 1000"),
                        (dict(max_read_alns=0), "kc_close_gaps: max_read_alns 0 outside 2 .. 64"),
                        (dict(flags=0x8000), "kc_close_gaps: unknown flags 0x8000")]
    for kw, text in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert text.encode() in L.kc_last_error(), (kw, L.kc_last_error())
        try:
            M.close_gaps(*case.args(), **kw)
        except M.BadArg as e:
            assert str(e).encode() in L.kc_last_error(), (str(e), L.kc_last_error())  # the model names the same values
        else:
            raise AssertionError("the model took %r" % (kw,))
    # in range, the corners included, the call gets as far as the NULL context and leaves the text alone
    for kw in GOOD_PARAMS + [{}]:
        assert call(**kw) == _lib.KC_ERR_INVALID_ARG, kw
        assert b"unknown flags 0x8000" in L.kc_last_error(), kw
    # the parameters and the size are required
    p = _lib.kc_close_params(**GOOD)
    head = (None, None, None, 0, None, 0, case.scaffolds.ctypes.data, 1, case.members.ctypes.data, 0)
    assert L.kc_close_gaps(*head, None, None, 0, None, None, None, None, C.byref(nb), None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_close_gaps(*head, C.byref(p), None, 0, None, None, None, None, None, None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_close_gaps(*head, C.byref(p), None, 0, None, None, None, None, C.byref(nb), C.byref(st)) == _lib.KC_ERR_INVALID_ARG  # no context
    assert (nb.value, st.members, st.disputed_cols) == (7, 7, 7)
    assert (seqs == 0xAB).all() and (offs == 0xABAB).all() and (scafs == 0xAB).all() and (members == 0xAB).all() and (closures == 0xAB).all()
