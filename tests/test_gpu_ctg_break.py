"""kc_ctg_break on the device equals tests/break_model.py byte for byte -- block, offsets, depths, pieces, breaks, tracks and
statistics -- on the forged-record cases of tests/break_cases.py; never against a second device run.  With
T = BREAK_TILE = 2048 the shapes are the smallest at which the kernels can go wrong: blocks of T - 1, T, T + 1 and 3T + 1 bytes; a
run ending on a tile's last byte, one starting on a tile's first, one over three tiles; a cut whose m is a tile's first byte; a
break in a contig whose separator is a tile's last byte; contigs of 2 * margin and 2 * margin + 1 bases; 300 empty contigs in a
row; 5000 short contigs around one of 300 020 bases; 65 535, 65 536 and 70 000 spanning pairs and discordant mates on a column;
0, 1, 17 and 4097 breaks in the gather.  The model's answers are computed once (break_cases.expected) and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import break_cases as BC
import break_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

K = 21
NAMES = sorted(BC.BUILDERS)
PAD = 64


def counter(c, **kw):
    """a counter that holds the case's contigs as its index"""
    kc = pkg.KmerCounter(K, **kw)
    kc.index_contigs(*c.contig_block())
    return kc


def host(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def same(got, want, depths=True, tracks=True):
    seqs, offs, dep, pieces, brk, stats, tr = got
    assert host(seqs).tobytes() == want[0]
    assert (host(offs).view(np.uint64) == want[1]).all()
    assert (dep is not None) == depths and (tr is not None) == tracks
    if depths:
        assert (host(dep).view(np.uint16) == want[2]).all(), np.flatnonzero(host(dep).view(np.uint16) != want[2])[:10]
    assert host(pieces).view(M.PIECE_DTYPE).tobytes() == want[3].tobytes()
    assert host(brk).view(M.BREAK_DTYPE).tobytes() == want[4].tobytes(), (host(brk).view(M.BREAK_DTYPE)[:5], want[4][:5])
    assert stats == want[5]
    if tracks:
        for g, w in zip(tr, want[6]):
            assert (host(g).view(np.uint16) == w).all(), np.flatnonzero(host(g).view(np.uint16) != w)[:10]


def records(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def args(c, device, depths=True, alns=None, pairs=None):
    """(offsets, gap_alns, pairs), depths of a case on either side"""
    alns, pairs = c.alns if alns is None else alns, c.pairs if pairs is None else pairs
    d = c.depths() if depths else None
    if not device:
        return (c.offsets, alns, pairs), d
    return (torch.from_numpy(c.offsets.astype(np.int64)).cuda(), records(alns), records(pairs)), (None if d is None else torch.from_numpy(d.view(np.int16)).cuda())


def call(kc, c, device, depths=True, tracks=True, **over):
    a, d = args(c, device, depths)
    return kc.break_contigs(*a, depths=d, tracks=tracks, **dict(c.kw, **over))


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_model(name, device):
    c = BC.case(name)
    with counter(c) as kc:
        same(call(kc, c, device), BC.expected(name))


def test_wrapper_without_depths_and_tracks_and_as_strings():
    c = BC.case("sep_tile_last")
    want = BC.expected("sep_tile_last")
    with counter(c) as kc:
        for device in (False, True):
            same(call(kc, c, device, depths=False, tracks=False), want, depths=False, tracks=False)
            same(call(kc, c, device, depths=False), want, depths=False)
        texts = want[0].decode().split("_")[:-1]
        assert pkg.break_strings(kc, *args(c, False)[0], **c.kw) == texts == kc.break_strings(*args(c, True)[0], **c.kw)
        assert len(texts) == len(c.contigs) + 3


@pytest.mark.parametrize("over", (dict(max_span=0), dict(max_span=1), dict(max_span=2), dict(max_span=3), dict(max_span=4), dict(max_span=5),
                                  dict(max_span=9, min_disc=0), dict(max_span=9, min_disc=1), dict(max_span=9, min_disc=3),
                                  dict(max_span=9, min_disc=4), dict(max_span=9, min_disc=5), dict(min_run=21), dict(min_run=20, margin=25),
                                  dict(one_mate=True)), ids=str)
def test_thresholds_at_under_and_over_the_columns_counts(over):
    """levels: span 0 .. 4 under disc 3 and disc 0 .. 4 under span 1; the model with the same parameters decides"""
    c = BC.case("levels")
    want = c.model(**over)
    with counter(c) as kc:
        same(call(kc, c, True, **over), want)


def test_one_mate_flag_on_the_classes():
    c = BC.case("classes")
    want = c.model(one_mate=True)
    assert want[5]["disc_mates"] == BC.expected("classes")[5]["disc_mates"] + 2
    with counter(c) as kc:
        same(call(kc, c, False, one_mate=True), want)
        same(call(kc, c, True, one_mate=True), want)


def test_shuffled_records_give_identical_bytes():
    c = BC.case("many")
    want = BC.expected("many")
    alns, pairs = c.alns, c.pairs
    with counter(c) as kc:
        for seed in (1, 2):
            perm = np.random.default_rng(seed).permutation(len(alns))
            inv = np.empty(len(alns), dtype=np.uint32)
            inv[perm] = np.arange(len(alns), dtype=np.uint32)
            p2 = pairs.copy()
            for f in ("aln0", "aln1"):
                has = pairs[f] != M.NO_ALN
                p2[f][has] = inv[pairs[f][has]]
            a, d = args(c, seed == 1, alns=alns[perm].copy(), pairs=p2)
            same(kc.break_contigs(*a, depths=d, tracks=True, **c.kw), want)


# ---- the raw call: exact arrays between canaries, every optional output, the sizes --------------------------------------
class Raw:
    """the arrays of one raw call, each exactly sized inside PAD bytes of 0xA5 on either side, on the host or the device"""

    def __init__(self, c, device, n_out, total, n_brk, depths=True):
        self.c, self.device = c, device
        nbytes = len(c.contig_block()[0])
        self.sizes = dict(seqs=total, offsets=(n_out + 1) * 8, depths=total * 2, pieces=n_out * 16, breaks=n_brk * 32, span=nbytes * 2, disc=nbytes * 2)
        self.buf = {k: self.canary(n) for k, n in self.sizes.items()}
        (self.offs, self.alns, self.pairs), self.din = args(c, device, depths)
        self.st, self.n_out, self.nbytes_out = _lib.kc_break_stats(), C.c_uint64(0xA5), C.c_uint64(0xA5)

    def canary(self, n):
        a = np.full(n + 2 * PAD, 0xA5, dtype=np.uint8)
        return torch.from_numpy(a).cuda() if self.device else a

    def ptr(self, k, shift=0):
        b = self.buf[k]
        return (b.data_ptr() if self.device else b.ctypes.data) + PAD + shift

    def inner(self, k):
        return host(self.buf[k])[PAD:PAD + self.sizes[k]]

    def untouched(self, only=None):
        return all((host(self.buf[k]) == 0xA5).all() for k in (only or self.buf))

    def margins_whole(self):
        return all((host(b)[:PAD] == 0xA5).all() and (host(b)[PAD + self.sizes[k]:] == 0xA5).all() for k, b in self.buf.items())

    def run(self, kc, capacity=None, break_capacity=None, skip=(), seqs=True, kw=None, shift=None):
        p = lambda x: None if x is None else (x.data_ptr() if self.device else x.ctypes.data)  # noqa: E731
        o = lambda k: None if k in skip else self.ptr(k, (shift or {}).get(k, 0))  # noqa: E731
        kw = dict(self.c.kw, **(kw or {}))
        prm = _lib.kc_break_params(kw["max_insert"], kw["max_span"], kw["min_disc"], kw["max_insert"] if kw["margin"] is None else kw["margin"],
                                   kw["min_run"], 1 if kw["one_mate"] else 0)
        if self.device:
            torch.cuda.synchronize()
        n_alns, n_pairs = len(self.c.alns), len(self.c.pairs)
        return pkg.lib().kc_ctg_break(kc._h, p(self.offs), 2 * n_pairs, p(self.alns) if n_alns else None, n_alns, p(self.pairs) if n_pairs else None,
                                      p(self.din), 1 if self.device else 0, C.byref(prm), o("seqs") if seqs else None,
                                      self.sizes["seqs"] if capacity is None else capacity, o("offsets"), o("depths"), o("pieces"), o("breaks"),
                                      self.sizes["breaks"] // 32 if break_capacity is None else break_capacity, o("span"), o("disc"),
                                      C.byref(self.n_out), C.byref(self.nbytes_out), C.byref(self.st))

    def got(self, skip=()):
        g = lambda k, dt: None if k in skip else self.inner(k).view(dt)  # noqa: E731
        return (self.inner("seqs"), g("offsets", np.uint64), g("depths", np.uint16), g("pieces", M.PIECE_DTYPE), g("breaks", M.BREAK_DTYPE),
                {f: int(getattr(self.st, f)) for f, _ in self.st._fields_ if f != "reserved"}, (g("span", np.uint16), g("disc", np.uint16)))


def raw_for(c, want, device, **kw):
    return Raw(c, device, len(want[1]) - 1, len(want[0]), len(want[4]), **kw)


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("name", ("cut_tile_first", "gather17", "empties"))
def test_exact_arrays_between_canaries(name, device):
    c, want = BC.case(name), BC.expected(name)
    with counter(c) as kc:
        r = raw_for(c, want, device)
        assert r.run(kc) == _lib.KC_OK, pkg.lib().kc_last_error()
        assert r.margins_whole()
        same(r.got(), want)
        assert (r.n_out.value, r.nbytes_out.value) == (len(want[1]) - 1, len(want[0])) and not any(r.st.reserved)


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_each_optional_output_null_in_turn(device):
    c, want = BC.case("size_3t+1"), BC.expected("size_3t+1")
    with counter(c) as kc:
        for k in ("offsets", "depths", "pieces", "breaks", "span", "disc"):
            r = raw_for(c, want, device)
            assert r.run(kc, skip=(k,)) == _lib.KC_OK, k
            assert r.untouched(only=(k,)) and r.margins_whole()
            got = list(r.got(skip=(k,)))
            for j, (name, w) in enumerate(zip(("seqs", "offsets", "depths", "pieces", "breaks"), want[:5])):
                if name != k:
                    assert np.asarray(got[j]).tobytes() == (w if isinstance(w, bytes) else w.tobytes()), (k, name)
            assert got[5] == want[5]
        r = raw_for(c, want, device, depths=False)  # no depths in: depths_out is not written
        assert r.run(kc) == _lib.KC_OK and r.untouched(only=("depths",)) and r.inner("seqs").tobytes() == want[0]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_size_query_and_capacities_one_short(device):
    c, want = BC.case("tile_first"), BC.expected("tile_first")
    n_out, total, n_brk = len(want[1]) - 1, len(want[0]), len(want[4])
    stats = lambda r: {f: int(getattr(r.st, f)) for f, _ in r.st._fields_ if f != "reserved"}  # noqa: E731
    with counter(c) as kc:
        r = raw_for(c, want, device)
        assert r.run(kc, seqs=False) == _lib.KC_OK  # the size query: the three and nothing else
        assert (r.n_out.value, r.nbytes_out.value) == (n_out, total) and stats(r) == want[5] and r.untouched()
        r = raw_for(c, want, device)
        assert r.run(kc, capacity=total - 1) == _lib.KC_ERR_CAPACITY
        assert ("kc_ctg_break: %d bytes, the array holds %d" % (total, total - 1)).encode() in pkg.lib().kc_last_error()
        assert (r.n_out.value, r.nbytes_out.value) == (n_out, total) and stats(r) == want[5] and r.untouched()
        r = raw_for(c, want, device)
        assert r.run(kc, break_capacity=n_brk - 1) == _lib.KC_ERR_CAPACITY
        assert ("kc_ctg_break: %d breaks, room for %d" % (n_brk, n_brk - 1)).encode() in pkg.lib().kc_last_error()
        assert (r.n_out.value, r.nbytes_out.value, r.st.pairs) == (0xA5, 0xA5, 0) and r.untouched()
        assert r.run(kc, break_capacity=0, skip=("breaks",)) == _lib.KC_OK  # no records asked for: no room needed
        assert r.inner("seqs").tobytes() == want[0]


def bad_call(kc, c, alns=None, pairs=None, offsets=None):
    """a host call with one array replaced; every output must stay as it was"""
    want = BC.expected("classes")
    r = raw_for(c, want, False)
    if alns is not None:
        r.alns = alns
    if pairs is not None:
        r.pairs = pairs
    if offsets is not None:
        r.offs = offsets
    rc = r.run(kc)
    assert r.untouched() and (r.n_out.value, r.nbytes_out.value, r.st.pairs) == (0xA5, 0xA5, 0)
    return rc, pkg.lib().kc_last_error()


def test_invalid_reads_records_and_pairs_name_the_lowest_and_write_nothing():
    c = BC.case("classes")
    n_reads, n_alns = len(c.offsets) - 1, len(c.alns)
    with counter(c) as kc:
        # ---- reads: one over the limit, decreasing offsets; alone and at two indices; a bad read comes before a bad record
        for grow, where in (((4,), 4), ((9, 4), 4)):
            offs = c.offsets.copy()
            for i in grow:
                offs[i + 1:] += 1100
            bad = c.alns.copy()
            bad[0]["ctg"] = 99
            rc, msg = bad_call(kc, c, offsets=offs, alns=bad)
            assert rc == _lib.KC_ERR_INVALID_ARG and (b"kc_ctg_break: read %d is longer than 1024 bases" % where) in msg, msg
        offs = c.offsets.copy()
        offs[7] = offs[6] - 1
        rc, msg = bad_call(kc, c, offsets=offs)
        assert rc == _lib.KC_ERR_INVALID_ARG and b"kc_ctg_break: read 6 is longer" in msg, msg
        # ---- records: every kind of invalid record, alone and with a later one; a bad record comes before a bad pair
        third = c.alns[3]
        for field, value in (("read", n_reads), ("ctg", 3), ("cstop", 10 ** 6), ("cstart", int(third["cstop"])), ("rstop", 11), ("rstart", 11),
                             ("orient", 2), ("kind", 3), ("rstop", 1025)):
            for later in (False, True):
                bad = c.alns.copy()
                bad[3][field] = value
                if later:
                    bad[8]["ctg"] = 7
                pr = c.pairs.copy()
                pr[0]["aln0"] = n_alns
                rc, msg = bad_call(kc, c, alns=bad, pairs=pr)
                assert rc == _lib.KC_ERR_INVALID_ARG and b"kc_ctg_break: record 3 is not a valid kc_gap_aln for this index and these reads" in msg, (field, msg)
        # ---- pairs: out of range, another read's record, a record of kind KC_GAP_NONE
        for p, field, value in ((2, "aln0", n_alns), (2, "aln1", int(c.pairs[3]["aln1"])), (5, "aln0", int(c.pairs[5]["aln1"]))):
            for later in (False, True):
                pr = c.pairs.copy()
                pr[p][field] = value
                if later:
                    pr[9]["aln1"] = n_alns + 5
                rc, msg = bad_call(kc, c, pairs=pr)
                assert rc == _lib.KC_ERR_INVALID_ARG and (b"kc_ctg_break: pair %d names a record" % p) in msg, (p, field, msg)
        bad = c.alns.copy()
        i = int(c.pairs[1]["aln1"])
        bad[i]["kind"] = 2
        rc, msg = bad_call(kc, c, alns=bad)
        assert rc == _lib.KC_ERR_INVALID_ARG and b"kc_ctg_break: pair 1 names a record" in msg, msg
        same(call(kc, c, False), BC.expected("classes"))  # and the counter still answers


def test_misaligned_device_arrays_no_index_and_null_arrays():
    c, want = BC.case("classes"), BC.expected("classes")
    L = pkg.lib()
    with pkg.KmerCounter(K) as kc:  # no index
        r = raw_for(c, want, False)
        assert r.run(kc) == _lib.KC_ERR_STATE and b"kc_ctg_break: no contig index (kc_ctg_index_build)" in L.kc_last_error() and r.untouched()
    with counter(c) as kc:
        for k, message in (("pieces", b"a device record array is 16-byte aligned"), ("breaks", b"a device record array is 16-byte aligned"),
                           ("offsets", b"device offsets are 8-byte aligned"), ("depths", b"depths and tracks 2-byte"),
                           ("span", b"depths and tracks 2-byte"), ("disc", b"depths and tracks 2-byte")):
            r = raw_for(c, want, True)
            assert r.run(kc, shift={k: 1 if k in ("depths", "span", "disc") else 4}) == _lib.KC_ERR_INVALID_ARG, k
            assert message in L.kc_last_error() and r.untouched()
        r = raw_for(c, want, True)  # the block itself may lie anywhere: every chunk but the ends is still one aligned store
        r.sizes["seqs"] += 3
        r.buf["seqs"] = r.canary(r.sizes["seqs"])
        assert r.run(kc, shift={"seqs": 3}, capacity=len(want[0])) == _lib.KC_OK
        whole = host(r.buf["seqs"])
        assert whole[PAD + 3:PAD + 3 + len(want[0])].tobytes() == want[0] and (whole[:PAD + 3] == 0xA5).all() and (whole[PAD + 3 + len(want[0]):] == 0xA5).all()
        r = raw_for(c, want, False)
        r.pairs = None
        prm = _lib.kc_break_params(40, 0, 1, 3, 1, 0)
        assert L.kc_ctg_break(kc._h, r.offs.ctypes.data, len(r.offs) - 1, r.alns.ctypes.data, len(r.alns), None, None, 0, C.byref(prm), None, 0, None,
                              None, None, None, 0, None, None, C.byref(r.n_out), C.byref(r.nbytes_out), None) == _lib.KC_ERR_INVALID_ARG
        assert b"kc_ctg_break: pairs is NULL" in L.kc_last_error()


def test_two_ranks_break_alike():
    c = BC.case("sep_tile_last")
    with counter(c, rank_me=1, rank_n=2) as kc:
        same(call(kc, c, True), BC.expected("sep_tile_last"))


def test_kernel_names_and_launch_counts():
    c = BC.case("cut_tile_first")
    with counter(c, time_kernels=True) as kc:
        kc.kernel_times(clear=True)
        same(call(kc, c, True), BC.expected("cut_tile_first"))
        t = {k: v[0] for k, v in kc.kernel_times().items() if v[0]}
    # the wrapper asks for the sizes first: every pass up to the count runs twice, what writes once
    assert t == {"kc_align_lengths_kernel<break>": 2, "kc_depth_check_kernel<break>": 2, "kc_lassm_pair_check_kernel<break>": 2, "kc_break_mark_kernel": 2,
                 "kc_break_tile_sums_kernel": 2, "kc_break_scan_kernel": 2, "kc_break_rescan_kernel": 2, "kc_break_tile_max_kernel": 2,
                 "kc_break_runs_kernel<count>": 2, "kc_break_scan_kernel<runs>": 2, "kc_break_runs_kernel<write>": 2, "kc_break_records_kernel": 2,
                 "kc_break_gather_kernel": 1, "kc_break_gather_kernel<depths>": 1, "kc_break_tracks_kernel": 2}, t


def test_index_results_and_earlier_calls_are_unchanged_afterwards():
    c = BC.case("sep_tile_last")
    rng = np.random.default_rng(5)
    reads = ["".join("ACGT"[x] for x in rng.integers(0, 4, 80)) for _ in range(40)]
    b = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    offs = np.arange(41, dtype=np.uint64) * 80
    with pkg.KmerCounter(K, dmin_thres=1) as kc:
        kc.submit_reads(b, np.full(len(b), 73, dtype=np.uint8), offs)
        before = [x.copy() for x in kc.sorted_results()]
        kc.index_contigs(*c.contig_block())
        info = kc.contig_index_info()
        rb = np.frombuffer(c.contigs[2][100:900].encode(), dtype=np.uint8).copy()
        ro = np.arange(11, dtype=np.uint64) * 80
        aligned = kc.align_reads(rb, ro)
        first = call(kc, c, False)
        same(first, BC.expected("sep_tile_last"))
        same(call(kc, c, True), BC.expected("sep_tile_last"))  # a second call on the same index: the first changed nothing it reads
        assert kc.contig_index_info() == info
        again = kc.align_reads(rb, ro)
        assert again[0].tobytes() == aligned[0].tobytes() and again[2] == aligned[2] and len(aligned[0]) >= 1
        assert all((x == y).all() for x, y in zip(before, kc.sorted_results()))
        # the new block is a block: the index takes it as it is
        kc.index_contigs(first[0], first[1])
        assert kc.contig_index_info() == (len(first[0]), len(first[1]) - 1)
