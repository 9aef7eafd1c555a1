"""kc_seq_kmer_depths and kc_count_spectrum are exported, their parameters, records and statistics have the layout the header
states, the Python defaults are the model's, and every range that needs no device is refused in front of the context, by the
values kc_last_error names (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import kdepth_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib, kcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kcount_mi355.h")).read()

C_TYPES = {"uint64_t": 8, "uint32_t": 4, "uint16_t": 2, "uint8_t": 1}


def header_layout(name):
    """[(field, offset)] and the size of a struct of fixed-width integers, from the header's text (natural alignment)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    at, fields, widest = 0, [], 1
    for ctype, names in re.findall(r"(u?int\d+_t)\s+([^;]+);", body):
        size = C_TYPES[ctype]
        widest = max(widest, size)
        for decl in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", decl)
            at = (at + size - 1) // size * size
            fields.append((m.group(1), at))
            at += size * int(m.group(2) or 1)
    return fields, (at + widest - 1) // widest * widest


def test_symbols_are_exported():
    L = pkg.lib()
    assert L.kc_seq_kmer_depths.restype is C.c_int and len(L.kc_seq_kmer_depths.argtypes) == 10
    assert L.kc_count_spectrum.restype is C.c_int and len(L.kc_count_spectrum.argtypes) == 4
    for name in ("kmer_depths", "contig_kmer_depths", "count_spectrum"):
        assert callable(getattr(kcount.KmerCounter, name))
    assert callable(pkg.format_spectrum) and L.kc_abi_version() == 1


def test_layouts_constants_and_defaults():
    for name, size in (("kc_kdepth_params", 32), ("kc_kdepth_rec", 32), ("kc_kdepth_stats", 64), ("kc_spectrum_stats", 64)):
        struct = getattr(_lib, name)
        fields, total = header_layout(name)
        assert total == size == C.sizeof(struct), name
        assert fields == [(n, getattr(struct, n).offset) for n, _ in struct._fields_], name
    want = [("sum", 0), ("windows", 8), ("present", 12), ("solid", 16), ("min_count", 20), ("max_count", 22), ("mean", 24)]
    for dtype in (M.REC_DTYPE, kcount.KDEPTH_DTYPE):
        assert dtype.itemsize == 32 and [(n, dtype.fields[n][1]) for n in dtype.names] == want + [("pad", 26)]
    assert header_layout("kc_kdepth_rec")[0] == want + [("reserved", 26)]
    assert [n for n, _ in _lib.kc_kdepth_stats._fields_] == list(M.STATS) + ["reserved"]
    assert [n for n, _ in _lib.kc_spectrum_stats._fields_] == list(M.SPECTRUM_STATS) + ["reserved"]
    assert _lib.KC_KDEPTH_FILL_MEAN == M.FILL_MEAN == 1 and re.search(r"#define KC_KDEPTH_FILL_MEAN 1u\b", HEADER)
    assert _lib.KC_SPECTRUM_BINS == M.BINS == 65536 and re.search(r"#define KC_SPECTRUM_BINS 65536\b", HEADER)
    sig = inspect.signature(kcount.KmerCounter.kmer_depths).parameters
    assert list(sig)[1:] == ["seqs", "offsets", "min_count", "fill_mean", "with_track", "with_records"]
    assert [sig[n].default for n in list(sig)[3:]] == [0, False, True, True]
    model = inspect.signature(M.kmer_depths).parameters
    assert [(n, model[n].default) for n in ("min_count", "fill_mean")] == [(n, sig[n].default) for n in ("min_count", "fill_mean")]
    assert list(inspect.signature(kcount.KmerCounter.contig_kmer_depths).parameters)[1:] == ["seqs", "offsets"]
    hist = np.zeros(M.BINS, np.uint64)
    hist[[2, 7, 65535]] = 5, 1, 3
    assert pkg.format_spectrum(hist) == M.format_spectrum(hist) == "2 5\n7 1\n65535 3\n"


def test_range_checks_come_before_the_context_and_write_nothing():
    L = pkg.lib()
    seqs, offsets = M.block(["ACGT", "GGNCA", "T"])
    track = np.full(len(seqs), 0xA5A5, dtype=np.uint16)
    recs = np.full(3 * 32, 0xA5, dtype=np.uint8)
    st = _lib.kc_kdepth_stats(seqs=7, longest=7)

    def depths(params=True, seqs_=seqs.ctypes.data, offsets_=offsets.ctypes.data, **kw):
        p = _lib.kc_kdepth_params(**kw)
        return L.kc_seq_kmer_depths(None, seqs_, len(seqs), offsets_, 3, 0, C.byref(p) if params else None, track.ctypes.data, recs.ctypes.data,
                                    C.byref(st))

    def reserved(at, value):
        r = (C.c_uint32 * 6)()
        r[at] = value
        return r

    bad = [(lambda: depths(flags=2), "kc_seq_kmer_depths: unknown flags 0x2"),
           (lambda: depths(flags=0x80000001), "kc_seq_kmer_depths: unknown flags 0x80000000"),
           (lambda: depths(reserved=reserved(0, 1)), "kc_seq_kmer_depths: reserved[0] is 1, not zero"),
           (lambda: depths(reserved=reserved(5, 9)), "kc_seq_kmer_depths: reserved[5] is 9, not zero"),
           (lambda: depths(min_count=65536), "kc_seq_kmer_depths: min_count is 65536, at most 65535"),
           (lambda: depths(params=False), "kc_seq_kmer_depths: params is NULL"),
           (lambda: depths(offsets_=None), "kc_seq_kmer_depths: offsets is NULL"),
           (lambda: depths(seqs_=None), "kc_seq_kmer_depths: seqs is NULL with 10 bytes"),
           (lambda: depths(), "kc_seq_kmer_depths: ctx is NULL"),
           (lambda: depths(min_count=65535, flags=1), "kc_seq_kmer_depths: ctx is NULL"),  # in range: as far as the context
           (lambda: L.kc_count_spectrum(None, None, 0, None), "kc_count_spectrum: hist and stats are both NULL"),
           (lambda: L.kc_count_spectrum(None, track.ctypes.data, 0, None), "kc_count_spectrum: ctx is NULL")]
    for call, message in bad:
        L.kc_scaffold(None, None, 0, 0, None, None, 0, None, None, None, None, None, None, None)  # leaves another text behind
        assert call() == _lib.KC_ERR_INVALID_ARG, message
        assert message.encode() in L.kc_last_error(), (message, L.kc_last_error())
    assert (st.seqs, st.longest, st.windows) == (7, 7, 0)
    assert (track == 0xA5A5).all() and (recs == 0xA5).all()
