"""kc_ctg_polish on the device equals tests/polish_model.py byte for byte -- block, counts, contig records, fixes and
statistics -- on the constructions of tests/polish_cases.py.  With T = POLISH_TILE = 1024 the shapes are
the smallest that still reach every path: a contig of 2T + 37 bases with records that start at T - 1, T, T - L + 1 and 2T - 1
and a 1024-base read across two tile boundaries, a 21-base contig and a separator in mid-tile, two contigs in one tile and a
partial last tile ("tiles"); both strands with qualities around min_qual, lower case and N ("strands"); every column outcome at
its bound ("columns"); every record class ("classes"); 66 000 records on one column range, which saturates the counts
("deep"); a block past 2^16 bytes, three radix passes ("long"); no placed record and no record at all.  The model's answers
are computed once (polish_cases.expected) and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import polish_cases as PC
import polish_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

K = 21
NAMES = sorted(PC.BUILDERS)


def counter(c, **kw):
    """a counter that holds the case's contigs as its index"""
    kc = pkg.KmerCounter(K, qual_offset=PC.QUAL_OFFSET, **kw)
    kc.index_contigs(*c.contig_block())
    return kc


def host(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def same(got, want, counts=True, records=True, fixes=True):
    out, cnt, recs, fx, stats = got
    assert host(out).tobytes() == want[0], np.flatnonzero(host(out) != np.frombuffer(want[0], dtype=np.uint8))[:10]
    assert (cnt is not None) == counts and (recs is not None) == records and (fx is not None) == fixes
    if counts:
        c = host(cnt).view(np.uint16).reshape(-1, 4)
        assert (c == want[1]).all(), np.flatnonzero((c != want[1]).any(axis=1))[:10]
    if records:
        r = host(recs).view(M.CTG_DTYPE)
        for name in M.CTG_DTYPE.names:
            assert (r[name] == want[2][name]).all(), (name, r[name], want[2][name])
    if fixes:
        f = host(fx).view(M.FIX_DTYPE)
        assert len(f) == len(want[3])
        for name in M.FIX_DTYPE.names:
            assert (f[name] == want[3][name]).all(), (name, np.flatnonzero(f[name] != want[3][name])[:10])
    assert stats == want[4]


def args(c, device, quals=True):
    """(bases, offsets, gap_alns), quals of a case on either side"""
    b, offs, q = c.block()
    alns = c.alns
    if not device:
        return (b, offs, alns), (q if quals else None)
    dev = (torch.from_numpy(b).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(alns.view(np.uint8).reshape(-1).copy()).cuda())
    return dev, (torch.from_numpy(q).cuda() if quals else None)


def call(kc, c, device, **over):
    a, q = args(c, device)
    kw = dict(c.kw, **over)
    return kc.polish_contigs(*a, quals=q, with_counts=True, **kw)


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_model(name, device):
    c = PC.case(name)
    with counter(c) as kc:
        same(call(kc, c, device), PC.expected(name))


def test_every_optional_output_left_out_in_turn():
    c = PC.case("tiles")
    want = PC.expected("tiles")
    with counter(c) as kc:
        for device in (False, True):
            a, q = args(c, device)
            same(kc.polish_contigs(*a, quals=q, **c.kw), want, counts=False)
            same(kc.polish_contigs(*a, quals=q, with_records=False, **c.kw), want, counts=False, records=False)
            same(kc.polish_contigs(*a, quals=q, with_fixes=False, with_counts=True, **c.kw), want, fixes=False)
            same(kc.polish_contigs(*a, quals=q, with_records=False, with_fixes=False, **c.kw), want, counts=False, records=False, fixes=False)
        assert pkg.polish_strings(kc, *args(c, False)[0], **c.kw) == want[0].decode().split("_")[:-1] == kc.polish_strings(*args(c, True)[0], **c.kw)


def test_variants_of_the_parameters():
    """edge_clip inside the contig and up to its greatest value, no qualities, no gate, best records only or not"""
    with counter(PC.case("tiles")) as kc:
        c = PC.case("tiles")
        for clip in (30, 1024):
            want = M.polish(c.contigs, c.reads, c.alns, quals=c.quals, **dict(c.kw, edge_clip=clip))
            same(call(kc, c, True, edge_clip=clip), want)
    c = PC.case("strands")
    with counter(c) as kc:
        gated = PC.expected("strands")
        free = M.polish(c.contigs, c.reads, c.alns, quals=None, **c.kw)
        assert free[4]["votes"] > gated[4]["votes"]
        a, _ = args(c, False)
        same(kc.polish_contigs(*a, quals=None, with_counts=True, **c.kw), free)
        same(call(kc, c, True, min_qual=0), free)
        same(call(kc, c, True, min_qual=21), M.polish(c.contigs, c.reads, c.alns, quals=c.quals, **dict(c.kw, min_qual=21)))
    c = PC.case("classes")
    with counter(c) as kc:
        for over in (dict(best_only=False), dict(best_only=False, edge_clip=0), dict(max_mismatches=4), dict(max_mismatches=2)):
            same(call(kc, c, False, **over), M.polish(c.contigs, c.reads, c.alns, quals=c.quals, **dict(c.kw, **over)))


def test_two_orders_of_the_records_give_identical_bytes():
    c = PC.case("long")
    want = PC.expected("long")
    b, offs, q = c.block()
    rows = c.alns
    with counter(c) as kc:
        for seed in (1, 2):
            perm = np.random.default_rng(seed).permutation(len(rows))
            same(kc.polish_contigs(b, offs, rows[perm].copy(), quals=q, with_counts=True, **c.kw), want)
        assert want[4]["sort_passes"] == 3


def raw_call(kc, c, out, counts, ctgs, fixes, capacity, st=None, alns=None, nreads=None):
    b, offs, _ = c.block()
    alns = c.alns if alns is None else alns
    kw = dict(M.DEFAULTS, **c.kw)
    prm = _lib.kc_polish_params(kw["min_score"], kw["min_len"], kw["edge_clip"], kw["max_mismatches"], kw["min_depth"], kw["min_permille"],
                                kw["min_qual"], 1 if kw["best_only"] else 0)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return pkg.lib().kc_ctg_polish(kc._h, b.ctypes.data, None, offs.ctypes.data, len(offs) - 1 if nreads is None else nreads, ptr(alns) if len(alns) else None,
                                   len(alns), 0, C.byref(prm), ptr(out), ptr(counts), ptr(ctgs), ptr(fixes), capacity, None if st is None else C.byref(st))


def test_exact_capacities_between_canaries_and_one_fix_short():
    c = PC.case("classes")
    want = M.polish(c.contigs, c.reads, c.alns, quals=None, **c.kw)
    nbytes, n_ctgs, n_fix = len(want[0]), len(c.contigs), len(want[3])
    assert n_fix >= 4
    pad = 64
    canary = lambda n, dtype: np.full(n * np.dtype(dtype).itemsize + 2 * pad, 0xA5, dtype=np.uint8)  # noqa: E731
    with counter(c) as kc:
        out, counts, ctgs, fixes = canary(nbytes, np.uint8), canary(nbytes * 4, np.uint16), canary(n_ctgs, M.CTG_DTYPE), canary(n_fix, M.FIX_DTYPE)
        inner = lambda a: a[pad:len(a) - pad]  # noqa: E731
        st = _lib.kc_polish_stats()
        # one fix short: KC_ERR_CAPACITY, the count named, and nothing written through any pointer
        assert raw_call(kc, c, inner(out), inner(counts), inner(ctgs), inner(fixes), n_fix - 1, st) == _lib.KC_ERR_CAPACITY
        assert ("kc_ctg_polish: %d fixes, room for %d" % (n_fix, n_fix - 1)).encode() in pkg.lib().kc_last_error()
        assert all((a == 0xA5).all() for a in (out, counts, ctgs, fixes)) and st.records == 0
        # exactly enough: every array whole, its neighbours untouched
        assert raw_call(kc, c, inner(out), inner(counts), inner(ctgs), inner(fixes), n_fix, st) == _lib.KC_OK
        for a in (out, counts, ctgs, fixes):
            assert (a[:pad] == 0xA5).all() and (a[len(a) - pad:] == 0xA5).all()
        got = (inner(out), inner(counts).view(np.uint16).reshape(-1, 4), inner(ctgs).view(M.CTG_DTYPE), inner(fixes).view(M.FIX_DTYPE),
               {f: int(getattr(st, f)) for f, _ in st._fields_})
        same(got, want)
        # no statistics asked for, no fixes: no capacity needed
        assert raw_call(kc, c, inner(out), None, None, None, 0) == _lib.KC_OK and inner(out).tobytes() == want[0]


def test_errors_name_their_cause_and_write_nothing():
    c = PC.case("classes")
    L = pkg.lib()
    nbytes = sum(len(x) + 1 for x in c.contigs)
    out, fixes = np.full(nbytes, 0xA5, dtype=np.uint8), np.full(nbytes * 16, 0xA5, dtype=np.uint8)
    with pkg.KmerCounter(K) as kc:  # no index
        assert raw_call(kc, c, out, None, None, fixes, nbytes) == _lib.KC_ERR_STATE
        assert b"kc_ctg_polish: no contig index (kc_ctg_index_build)" in L.kc_last_error()
    with counter(c) as kc:
        for field, value in (("read", len(c.reads)), ("ctg", 1), ("cstop", 501), ("rstop", 61), ("orient", 2), ("kind", 3)):
            rows = c.alns
            rows[5][field] = value
            rows[9]["ctg"] = 7  # a later bad record is not the one named
            assert raw_call(kc, c, out, None, None, fixes, nbytes, alns=rows) == _lib.KC_ERR_INVALID_ARG, field
            assert b"kc_ctg_polish: record 5 is not a valid kc_gap_aln for this index and these reads" in L.kc_last_error(), (field, L.kc_last_error())
        assert raw_call(kc, c, None, None, None, None, 0) == _lib.KC_ERR_INVALID_ARG and b"kc_ctg_polish: out is NULL" in L.kc_last_error()
        assert (out == 0xA5).all() and (fixes == 0xA5).all()
        with pytest.raises(_lib.KcError) as e:
            kc.polish_contigs(*args(c, True)[0], with_fixes=3, **c.kw)
        assert e.value.status == _lib.KC_ERR_CAPACITY


def test_index_results_and_lookup_are_unchanged_afterwards():
    c = PC.case("strands")
    rng = np.random.default_rng(5)
    reads = ["".join("ACGT"[x] for x in rng.integers(0, 4, 80)) for _ in range(40)]
    b = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    offs = np.arange(41, dtype=np.uint64) * 80
    with pkg.KmerCounter(K, qual_offset=PC.QUAL_OFFSET, dmin_thres=1) as kc:
        kc.submit_reads(b, np.full(len(b), 73, dtype=np.uint8), offs)
        before = [x.copy() for x in kc.sorted_results()]
        kc.index_contigs(*c.contig_block())
        info = kc.contig_index_info()
        aligned = kc.align_reads(*c.block()[:2])
        same(call(kc, c, False), PC.expected("strands"))
        same(call(kc, c, True), PC.expected("strands"))  # a second call on the same index: the first changed nothing it reads
        assert kc.contig_index_info() == info
        again = kc.align_reads(*c.block()[:2])
        assert again[0].tobytes() == aligned[0].tobytes() and again[2] == aligned[2]
        after = kc.sorted_results()
        assert all((x == y).all() for x, y in zip(before, after))
        keys = before[0][:16]
        found = kc.lookup(keys)
        assert (np.asarray(found[0]) == before[1][:16]).all()


def test_two_ranks_polish_alike():
    c = PC.case("columns")
    with counter(c, rank_me=1, rank_n=2) as kc:
        same(call(kc, c, True), PC.expected("columns"))
