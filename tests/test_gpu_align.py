"""kc_ctg_index_build / kc_align_reads (csrc/kc_align.hpp) against the host model tests/align_model.py, byte for byte:
the records, read_first and both statistics structs on the same inputs.  The model is never replaced by a second device
run.

Every device call goes through device_align: a size query, then the call with arrays of exactly that size inside
canaries.  The reads kernel is instantiated for 1, 3, 8 and 16 windows a lane and the host picks the class by the
longest read of a call, so the window-count cases run one call each: 0, 1, 63, 64 (class 1), 65, 128, 129 (class 3),
256, 257 (class 8) and everything up to L = 1024 (class 16) sit on either side of every boundary."""
import ctypes as C

import numpy as np
import pytest

import align_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

KEEP_ALL = M.KEEP_ALL


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def mutate(read, x):
    return read[:x] + "ACGT"[("ACGT".index(read[x]) + 1) % 4] + read[x + 1:]


def read_arrays(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), offs


def block_arrays(contigs):
    block, offsets = M.join_block(contigs)
    return np.frombuffer(block.encode(), dtype=np.uint8).copy(), np.array(offsets, dtype=np.uint64)


def stats_dict(st):
    return {n: int(getattr(st, n)) for n, _ in st._fields_}


def indexed(k, contigs, **kw):
    """a counter with the contigs indexed, and the model's index; the two index statistics agree"""
    kc = pkg.KmerCounter(k, **kw)
    ix = M.Index(*M.join_block(contigs), k)
    assert kc.index_contigs(*block_arrays(contigs)) == ix.stats
    return kc, ix


def raw_align(kc, pb, po, n, on_device, s, mm, pa, cap, pf):
    na, st = C.c_uint64(0), _lib.kc_align_stats()
    rc = pkg.lib().kc_align_reads(kc._h, pb, po, n, on_device, s, mm, pa, cap, pf, C.byref(na), C.byref(st))
    return rc, na.value, stats_dict(st)


def device_align(kc, reads, s=1, mm=KEEP_ALL, with_first=True, short_by=0):
    """size query, then the call on device arrays of exactly that size inside canaries: (records, read_first, stats).
    short_by = 1: the call with one record less room -- returns its status after checking that nothing was written."""
    import torch
    b, o = read_arrays(reads)
    d_b = torch.from_numpy(b).cuda()
    d_o = torch.from_numpy(o.view(np.int64)).cuda()
    torch.cuda.synchronize()
    pb, po, n = (d_b.data_ptr() if len(b) else None), d_o.data_ptr(), len(reads)
    rc, na, st = raw_align(kc, pb, po, n, 1, s, mm, None, 0, None)
    assert rc == 0
    PAD = 64  # bytes in front of and behind the records; entries around read_first
    d_a = torch.full((na * 32 + 2 * PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    d_f = torch.full((n + 1 + 2 * PAD,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc2, na2, st2 = raw_align(kc, pb, po, n, 1, s, mm, d_a.data_ptr() + PAD, na - short_by, d_f.data_ptr() + 8 * PAD if with_first else None)
    ha, hf = d_a.cpu().numpy(), d_f.cpu().numpy()
    if short_by:
        assert (ha == 0xAB).all() and (hf == -7).all(), "a call without room wrote something"
        assert (na2, st2) == (na, st)
        return rc2
    assert rc2 == 0 and (na2, st2) == (na, st), "a size query equals the call"
    assert (ha[:PAD] == 0xAB).all() and (ha[PAD + na * 32:] == 0xAB).all(), "a canary was written"
    assert (hf[:PAD] == -7).all() and (hf[PAD + (n + 1 if with_first else 0):] == -7).all(), "a canary was written"
    recs = ha[PAD:PAD + na * 32].copy().view(M.ALN_DTYPE)
    return recs, hf[PAD:PAD + n + 1].astype(np.uint64) if with_first else None, st


def compare(kc, ix, reads, s=1, mm=KEEP_ALL):
    want, want_first, want_st = M.align_reads(ix, reads, s, mm)
    got, got_first, got_st = device_align(kc, reads, s, mm)
    assert got_st == want_st
    assert (got_first == want_first).all()
    assert got.tobytes() == want.tobytes()
    return want, want_st


def cut(rng, ctg, L):
    a = int(rng.integers(0, len(ctg) - L + 1))
    return ctg[a:a + L]


# ---- key widths x windows per read ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32, 33, 77, 99])
def test_key_widths_and_windows_per_read(k):
    rng = np.random.default_rng(k)
    contigs = [rand_seq(rng, 1400 + 100 * u) for u in range(3)]
    kc, ix = indexed(k, contigs)
    assert ix.stats["repeated"] == 0
    with kc:
        want, st = compare(kc, ix, ["", contigs[0][:k - 1], "ACGT"[:min(4, k - 1)]])  # no window at all: L = 0, L < k
        assert len(want) == 0 and st["windows"] == 0
        for w in (1, 63, 64, 65, 128, 129, 256, 257, 1004):
            L = min(w + k - 1, 1024)  # 1004 windows are L = 1024 at k = 21; the longer k end at 1024 bases as well
            reads = []
            for u, ctg in enumerate(contigs):
                r = cut(rng, ctg, L)
                reads += [r, M.revcomp(r), mutate(r, L // 2), M.revcomp(mutate(r, L - 1))]
            reads.append(rand_seq(rng, L))
            want, st = compare(kc, ix, reads)
            assert st["reads_aligned"] >= 6 and st["perfect"] == 6
            assert int(want["seeds"].max()) == L - k + 1


@pytest.mark.parametrize("s", [1, 2, 4, 7, 21, 2000])
def test_seed_space(s):
    k = 21
    rng = np.random.default_rng(50 + s)
    contigs = [rand_seq(rng, 1300), rand_seq(rng, 1100)]
    kc, ix = indexed(k, contigs)
    with kc:
        for L in (150, 1024):
            reads = [cut(rng, contigs[0], L), M.revcomp(cut(rng, contigs[1], L)), mutate(cut(rng, contigs[1], L), 30), rand_seq(rng, L)]
            reads.append(contigs[0][100:100 + L // 2] + contigs[1][300:300 + L - L // 2])
            want, st = compare(kc, ix, reads, s=s)
            assert int(want["seeds"][0]) == len(range(0, L - k + 1, s))


# ---- geometry --------------------------------------------------------------------------------------------------------------
def test_geometry():
    k = 21
    rng = np.random.default_rng(7)
    c0, c2, c3 = rand_seq(rng, 500), rand_seq(rng, 400), rand_seq(rng, 600)
    c1 = rand_seq(rng, k)  # a contig of exactly k bases
    pieces = [rand_seq(rng, 34 + int(rng.integers(0, 20))) for _ in range(30)]
    contigs = [c0, "", c1, "", "", c2, c3, ""] + pieces + ["", rand_seq(rng, k - 1)]
    kc, ix = indexed(k, contigs)
    reads = [rand_seq(rng, 30) + c0[:120],                       # over the contig's start: d = -30
             c0[-100:] + rand_seq(rng, 50),                       # over its end
             rand_seq(rng, 60) + c1 + rand_seq(rng, 69),          # 150 bases over a contig of k
             c0[-75:] + c2[:75],                                  # spanning two contigs
             c3[100:175] + c3[185:260],                           # a deletion: two diagonals
             "".join(p[:34] for p in pieces),                     # 34-base pieces of 30 contigs: 30 candidates
             c2]                                                  # a whole contig
    reads += [M.revcomp(r) for r in reads]
    with kc:
        want, st = compare(kc, ix, reads)
        per_read = np.diff(M.align_reads(ix, reads)[1].astype(np.int64))
        assert list(per_read[:7]) == [1, 1, 1, 2, 2, 30, 1] and list(per_read[7:]) == list(per_read[:7])
        r0, r1, r2 = want[0], want[1], want[2]
        assert (int(r0["cstart"]), int(r0["rstart"]), int(r0["rstop"])) == (0, 30, 150)
        assert (int(r1["cstop"]), int(r1["rstart"]), int(r1["rstop"])) == (500, 0, 100)
        assert (int(r2["cstart"]), int(r2["cstop"]), int(r2["rstart"]), int(r2["rstop"]), int(r2["seeds"])) == (0, k, 60, 60 + k, 1)
        compare(kc, ix, reads, s=3, mm=0)


# ---- seeds -----------------------------------------------------------------------------------------------------------------
def test_repeats_ns_and_case():
    k = 21
    rng = np.random.default_rng(8)
    shared, twice = rand_seq(rng, k), rand_seq(rng, k)
    a = rand_seq(rng, 200) + shared + rand_seq(rng, 200)
    b = rand_seq(rng, 150) + M.revcomp(shared) + rand_seq(rng, 100)     # the same k-mer on the other strand of another contig
    c = rand_seq(rng, 90) + twice + rand_seq(rng, 60) + twice + rand_seq(rng, 80)  # twice in one contig
    d = rand_seq(rng, 120) + "N" + rand_seq(rng, 150)                   # an N in a contig: no window covers it
    contigs = [a, b, c, d]
    kc, ix = indexed(k, contigs)
    assert ix.stats["repeated"] == 2
    reads = ["NNNNN" + shared + "NNNNN",                                # its only hit is repeated: no record
             twice,
             a[180:260],                                                # a read over the repeated k-mer: fewer seeds, one record
             c[60:240],
             d[60:200],                                                 # over the contig's N: a mismatch by definition
             a[20:60] + "N" + a[61:140],                                # an N in the read
             a[20:140].lower(), M.revcomp(b[40:190]).lower(),           # lower-case bases are bases
             a[300:330] + "n-*" + a[333:400]]
    reads += [M.revcomp(r) for r in reads]
    with kc:
        want, st = compare(kc, ix, reads)
        first = M.align_reads(ix, reads)[1]
        assert first[1] == 0 and first[2] == 0 and st["repeated_hits"] > 0  # reads 0 and 1 give no record
        assert int(want[int(first[4])]["mismatches"]) == 1 and int(want[int(first[5])]["mismatches"]) == 1
        compare(kc, ix, reads, mm=0)


def test_palindromic_32mer():
    k = 32
    rng = np.random.default_rng(9)
    half = rand_seq(rng, 16)
    pal = half + M.revcomp(half)
    assert pal == M.revcomp(pal)
    contigs = [rand_seq(rng, 100) + pal + rand_seq(rng, 100), rand_seq(rng, 300)]
    kc, ix = indexed(k, contigs)
    assert ix.seeds[pal] is None and ix.stats["repeated"] == 1
    reads = [pal, "NNNNN" + pal + "nnnnn", contigs[0][60:200], M.revcomp(contigs[0][80:190])]
    with kc:
        want, st = compare(kc, ix, reads)
        assert st["repeated_hits"] == 4 and st["reads_aligned"] == 2


# ---- the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1, KEEP_ALL])
def test_max_mismatches(mm):
    k = 21
    rng = np.random.default_rng(10)
    contigs = [rand_seq(rng, 700), rand_seq(rng, 900)]
    kc, ix = indexed(k, contigs)
    r = contigs[1][200:350]
    reads = [r, mutate(r, 75), mutate(mutate(r, 40), 110), M.revcomp(mutate(r, 0)), M.revcomp(mutate(mutate(r, 0), 149)),
             contigs[0][:100] + rand_seq(rng, 50)]
    with kc:
        want, st = compare(kc, ix, reads, mm=mm)
        per_read = list(np.diff(M.align_reads(ix, reads, 1, mm)[1].astype(np.int64)))
        # exactly at the limit stays, one over goes
        assert per_read == {0: [1, 0, 0, 0, 0, 0], 1: [1, 1, 0, 1, 0, 0], KEEP_ALL: [1, 1, 1, 1, 1, 1]}[mm]


# ---- size ------------------------------------------------------------------------------------------------------------------
def test_one_long_contig_beside_five_thousand_short_ones():
    k = 21
    rng = np.random.default_rng(11)
    big = rand_seq(rng, 300020)
    small = [rand_seq(rng, int(n)) for n in rng.integers(25, 61, size=5000)]
    contigs = small[:2500] + [big] + small[2500:]
    kc, ix = indexed(k, contigs)
    reads = [cut(rng, big, 100) for _ in range(600)] + [M.revcomp(cut(rng, big, 150)) for _ in range(300)]
    reads += [small[int(i)] for i in rng.integers(0, 5000, size=600)]
    reads += [small[int(i)][-22:] + small[int(j)][:30] for i, j in rng.integers(0, 5000, size=(300, 2))]
    reads += [big[-80:] + rand_seq(rng, 20), rand_seq(rng, 20) + big[:80], small[0], small[-1], small[2499], small[2500]]
    with kc:
        want, st = compare(kc, ix, reads)
        assert st["alignments"] >= len(reads)


def test_a_hundred_thousand_reads():
    k = 21
    rng = np.random.default_rng(12)
    contigs = [rand_seq(rng, 400) for _ in range(40)]
    pool = [cut(rng, contigs[int(u)], 60) for u in rng.integers(0, 40, size=300)]
    pool += [M.revcomp(mutate(r, 30)) for r in pool[:100]]
    pool += [rand_seq(rng, 60) for _ in range(100)]  # these align nowhere
    for _ in range(60):  # and these three times: the windows at 0, 20 and 39 each come from another contig
        r = rand_seq(rng, 60)
        contigs += [rand_seq(rng, 30) + r[:21] + rand_seq(rng, 40), rand_seq(rng, 50) + r[20:41] + rand_seq(rng, 10),
                    rand_seq(rng, 5) + M.revcomp(r[39:]) + rand_seq(rng, 70)]
        pool.append(r)
    kc, ix = indexed(k, contigs)
    reads = [pool[int(i)] for i in rng.integers(0, len(pool), size=100000)]
    with kc:
        want, st = compare(kc, ix, reads)
        per_read = np.bincount(want["read"], minlength=len(reads))
        assert (per_read == 0).sum() > 5000 and (per_read == 3).sum() > 5000 and st["reads"] == 100000


# ---- the protocol ----------------------------------------------------------------------------------------------------------
def small_case(rng, k=21):
    contigs = [rand_seq(rng, 300), "", rand_seq(rng, 250)]
    reads = [contigs[0][10:160], M.revcomp(contigs[2][50:200]), contigs[0][250:] + contigs[2][:40], rand_seq(rng, 80), ""]
    return contigs, reads


def test_capacity_read_first_and_repeatability():
    rng = np.random.default_rng(13)
    contigs, reads = small_case(rng)
    kc, ix = indexed(21, contigs)
    with kc:
        want, st = compare(kc, ix, reads)
        assert len(want) == 4 and not want["pad"].any()
        assert device_align(kc, reads, short_by=1) == _lib.KC_ERR_CAPACITY  # one record short: nothing is written
        got, first, _ = device_align(kc, reads, with_first=False)  # read_first NULL
        assert first is None and got.tobytes() == want.tobytes()
        again, _, _ = device_align(kc, reads)  # the same call twice
        assert again.tobytes() == want.tobytes()
        # host inputs give the same bytes (the Python wrapper: numpy in, numpy out)
        h_alns, h_first, h_st = kc.align_reads(*read_arrays(reads))
        assert h_alns.tobytes() == want.tobytes() and h_st == st and (h_first == M.align_reads(ix, reads)[1]).all()
        h_alns, _, _ = kc.align_reads(*read_arrays(reads), seed_space=5, max_mismatches=0)
        assert h_alns.tobytes() == M.align_reads(ix, reads, 5, 0)[0].tobytes()
        # no reads
        rc, na, st0 = raw_align(kc, None, None, 0, 0, 1, KEEP_ALL, None, 0, None)
        assert (rc, na, st0["reads"]) == (0, 0, 0)


def test_names_and_launch_counts_in_the_kernel_times():
    rng = np.random.default_rng(13)
    contigs, reads = small_case(rng)
    kc, ix = indexed(21, contigs, time_kernels=True)
    with kc:
        kc.kernel_times(clear=True)
        alns, _, _ = kc.align_reads(*read_arrays(reads))  # a size query and the call
        assert len(alns) == 4
        t = kc.kernel_times()
    want = {"kc_align_lengths_kernel": 2, "kc_align_reads_kernel<count>": 2, "kc_align_scan_kernel": 2, "kc_align_reads_kernel<write>": 1}
    assert {n: c for n, (c, _) in t.items()} == want


def test_state_and_argument_errors():
    import torch
    rng = np.random.default_rng(14)
    contigs, reads = small_case(rng)
    b, o = read_arrays(reads)
    L = pkg.lib()
    with pkg.KmerCounter(21) as kc:
        def status():
            return raw_align(kc, b.ctypes.data, o.ctypes.data, len(reads), 0, 1, KEEP_ALL, None, 0, None)[0]
        assert status() == _lib.KC_ERR_STATE  # no index
        ix = M.Index(*M.join_block(contigs), 21)
        assert kc.index_contigs(*block_arrays(contigs)) == ix.stats
        assert status() == 0
        assert raw_align(kc, b.ctypes.data, o.ctypes.data, len(reads), 0, 0, KEEP_ALL, None, 0, None)[0] == _lib.KC_ERR_INVALID_ARG
        kc.clear_contig_index()
        assert status() == _lib.KC_ERR_STATE
        kc.index_contigs(*block_arrays(contigs))
        kc.reset()
        assert status() == _lib.KC_ERR_STATE  # kc_reset drops the index
        kc.index_contigs(*block_arrays(contigs))
        # a read over the limit, named
        lb, lo = read_arrays([reads[0], "A" * 1024, "C" * 1025, "G" * 2000])
        assert raw_align(kc, lb.ctypes.data, lo.ctypes.data, 4, 0, 1, KEEP_ALL, None, 0, None)[0] == _lib.KC_ERR_INVALID_ARG
        assert b"read 2" in L.kc_last_error()
        assert raw_align(kc, lb.ctypes.data, lo.ctypes.data, 2, 0, 1, KEEP_ALL, None, 0, None)[0] == 0
        # blocks the index refuses: the earlier index answers as before
        want = M.align_reads(ix, reads)[0].tobytes()
        blk, offs = block_arrays(contigs)
        bad = blk.copy()
        bad[17] = ord("x")
        st = _lib.kc_ctg_index_stats()
        assert L.kc_ctg_index_build(kc._h, bad.ctypes.data, len(bad), offs.ctypes.data, len(contigs), 0, C.byref(st)) == _lib.KC_ERR_BAD_BASE
        assert device_align(kc, reads)[0].tobytes() == want
        low = blk.copy()
        low[17] = ord("a")
        assert L.kc_ctg_index_build(kc._h, low.ctypes.data, len(low), offs.ctypes.data, len(contigs), 0, None) == _lib.KC_ERR_BAD_BASE
        for wrong in (offs + np.uint64(1), np.concatenate([offs[:1], offs[1:2] - np.uint64(1), offs[2:]]), offs[:-1].copy()):
            n = len(wrong) - 1
            assert L.kc_ctg_index_build(kc._h, blk.ctypes.data, len(blk), wrong.ctypes.data, n, 0, None) == _lib.KC_ERR_INVALID_ARG
        wild = offs.copy()
        wild[1] = np.uint64(1) << np.uint64(40)  # an offset far outside the block is compared, never followed
        assert L.kc_ctg_index_build(kc._h, blk.ctypes.data, len(blk), wild.ctypes.data, len(contigs), 0, None) == _lib.KC_ERR_INVALID_ARG
        assert L.kc_ctg_index_build(kc._h, blk.ctypes.data, 1 << 31, offs.ctypes.data, len(contigs), 0, None) == _lib.KC_ERR_CAPACITY
        assert device_align(kc, reads)[0].tobytes() == want
        # a rebuild replaces the index: other contigs, other answers; device tensors as input
        contigs2 = [contigs[2], rand_seq(rng, 100)]
        ix2 = M.Index(*M.join_block(contigs2), 21)
        blk2, offs2 = block_arrays(contigs2)
        assert kc.index_contigs(torch.from_numpy(blk2).cuda(), torch.from_numpy(offs2.view(np.int64)).cuda()) == ix2.stats
        compare(kc, ix2, reads)
        # no contigs at all is an index too
        assert kc.index_contigs(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)) == M.Index("", [0], 21).stats
        compare(kc, M.Index("", [0], 21), reads)


def test_a_rank_of_two_aligns():
    rng = np.random.default_rng(15)
    contigs, reads = small_case(rng)
    kc, ix = indexed(21, contigs, rank_me=1, rank_n=2)
    with kc:
        compare(kc, ix, reads)


def test_counting_is_untouched_and_the_loop_closes():
    """Count reads that cover a few chains, index the unitigs on the device, align the same reads: the device against the
    model run on unitig_strings(); results(), lookup() and unitigs() are the same before and after."""
    k, READ = 21, 200
    rng = np.random.default_rng(16)
    chains = [rand_seq(rng, m + k + 1) for m in (300, 64, 1000, 5)]
    reads, inside = [], []
    for seq in chains:
        for a in range(0, max(1, len(seq) - k - 1), READ - k - 1):
            r = seq[a:a + READ]
            reads += [r, r]
            inside += [a >= 1 and a + len(r) <= len(seq) - 1 and len(r) >= k] * 2
        reads += [seq[1:-1]] * 2  # the chain's whole interior (1020 bases at most)
        inside += [True] * 2
    b, o = read_arrays(reads)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(b, np.full(len(b), ord("I"), dtype=np.uint8), o)
        kc.finalize()
        strings = kc.unitig_strings()
        keys, counts, left, right = [np.array(x) for x in kc.sorted_results()]
        looked = [np.array(x) for x in kc.lookup(keys)]
        ix = M.Index(*M.join_block([s for s, _ in strings]), k)
        assert kc.index_unitigs() == ix.stats
        assert ix.stats["repeated"] == 0 and ix.stats["seeds"] == len(counts)  # every k-mer of a unitig is a seed
        want, st = compare(kc, ix, reads)
        first = M.align_reads(ix, reads)[1]
        for r, ok in enumerate(inside):
            if ok:  # an error-free read inside a chain: one perfect full-length record
                assert first[r + 1] - first[r] == 1
                a = want[int(first[r])]
                assert (int(a["mismatches"]), int(a["rstart"]), int(a["rstop"])) == (0, 0, len(reads[r]))
        assert sum(inside) == 16  # four windows of the longest chain and every chain's interior, twice each
        after = [np.array(x) for x in kc.sorted_results()]
        for x, y in zip((keys, counts, left, right), after):
            assert (x == y).all()
        for x, y in zip(looked, [np.array(x) for x in kc.lookup(keys)]):
            assert (x == y).all()
        assert kc.unitig_strings() == strings
