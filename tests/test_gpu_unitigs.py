"""kc_build_unitigs (csrc/kc_unitig.hpp) against the host model tests/unitig_model.py, byte for byte.

Every case counts reads built so that the result set has a known shape (substrings of chosen sequences, each submitted
two or three times, all of high quality), copies the context's OWN results to the host, runs the model on them and
compares the sequence block, the offsets, the k-mer sums, the depths and the statistics with what the device wrote.
Whether the results themselves are right is the business of the parity tests; the model is never replaced by a second
device run.

Shapes: chains of 1, 2, 3, 64, 65 and 4097 k-mers sit around the wave (64), the workgroup (256) and a round of the
pointer jumping (4096 = 2^12); circles of 2, 3, 64 and 5000 k-mers exercise the cycle search and its cut; one chain of
270 000 k-mers needs 19 rounds of jumping (2^18 < 270 000) beside about 2000 short ones."""
import ctypes as C

import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
import unitig_model as M
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

READ = 200  # bases of a read cut from a longer sequence


def arrays(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    b = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    return b, np.full(len(b), ord("I"), dtype=np.uint8), offs


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def cover(seq, k, times=2):
    """reads that give every k-mer of seq that has both neighbours there (positions 1 .. len - k - 1) both neighbours in
    a read, `times` times or more: windows of READ bases whose inner k-mers follow on one another"""
    step = READ - k - 1
    out = []
    for a in range(0, max(1, len(seq) - k - 1), step):
        out += [seq[a:a + READ]] * times
    return out


def chain(rng, m, k):
    """a random sequence with m k-mers that have both neighbours: one unitig of m k-mers, unless chance repeats a k-mer"""
    return rand_seq(rng, m + k + 1)


def circle_read(circle, k):
    """the circle written twice plus k + 1 bases: every cyclic k-mer has both neighbours, twice"""
    c = len(circle)
    return (circle * (2 + (k + 1) // c + 1))[:2 * c + k + 1]


def smallest_on_forward(circle, k):
    c = len(circle)
    ring = circle * (1 + k // c + 1)
    kmers = [ring[i:i + k] for i in range(c)]
    return min(M.canonical(x) for x in kmers) in kmers


def device_unitigs(kc, depths=True, sums=True):
    """size query, then the call with arrays of exactly that size inside canaries: numpy (seqs, depths, offsets, sums,
    stats dict)"""
    import torch
    L = pkg.lib()
    kc.finalize()  # (a call before kc_finalize is KC_ERR_STATE: test_state_errors)
    nu, nb, st = C.c_uint64(0), C.c_uint64(0), _lib.kc_unitig_stats()
    _lib.check(L.kc_build_unitigs(kc._h, None, 0, None, None, 0, None, C.byref(nu), C.byref(nb), C.byref(st)), "kc_build_unitigs")
    query = (nu.value, nb.value, {n: int(getattr(st, n)) for n, _ in st._fields_})
    PAD = 16
    d_seqs = torch.full((nb.value + 2 * PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    d_dep = torch.full((nb.value + 2 * PAD,), 0x5A5A, dtype=torch.int16, device="cuda")
    d_off = torch.full((nu.value + 1 + 2 * PAD,), -7, dtype=torch.int64, device="cuda")
    d_sum = torch.full((nu.value + 2 * PAD,), -9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nu2, nb2, st2 = C.c_uint64(0), C.c_uint64(0), _lib.kc_unitig_stats()
    _lib.check(L.kc_build_unitigs(kc._h, d_seqs.data_ptr() + PAD, nb.value, d_dep.data_ptr() + 2 * PAD if depths else None,
                                  d_off.data_ptr() + 8 * PAD, nu.value, d_sum.data_ptr() + 8 * PAD if sums else None, C.byref(nu2),
                                  C.byref(nb2), C.byref(st2)), "kc_build_unitigs")
    assert (nu2.value, nb2.value, {n: int(getattr(st2, n)) for n, _ in st2._fields_}) == query
    hs, hd, ho, hm = d_seqs.cpu().numpy(), d_dep.cpu().numpy().view(np.uint16), d_off.cpu().numpy(), d_sum.cpu().numpy()
    for a, fill, n in ((hs, 0xAB, nb.value), (hd, 0x5A5A, nb.value if depths else 0), (ho, -7, nu.value + 1), (hm, -9, nu.value if sums else 0)):
        assert (a[:PAD] == fill).all() and (a[PAD + n:] == fill).all(), "a canary was written"
        if n == 0:
            assert (a == fill).all()
    return (hs[PAD:PAD + nb.value].tobytes(), hd[PAD:PAD + nb.value].copy(), ho[PAD:PAD + nu.value + 1].astype(np.uint64),
            hm[PAD:PAD + nu.value].astype(np.uint64), query[2])


def model_of(kc):
    """the model on the context's own results: (units, stats, (seqs, depths, offsets, sums), R)"""
    keys, counts, left, right = kc.results()
    R = M.results_dict(keys, counts, left, right, kc.k)
    units, st = M.unitigs(R, kc.k)
    return units, st, M.block(units), R


def compare(kc):
    units, st, (seqs, depths, offsets, sums), R = model_of(kc)
    g_seqs, g_depths, g_offsets, g_sums, g_st = device_unitigs(kc)
    assert g_st == st
    assert len(g_seqs) == len(seqs) and g_seqs == seqs
    assert (g_offsets == offsets).all()
    assert (g_sums == sums).all()
    assert (g_depths == depths).all()
    return units, st, R


def counted(k, reads):
    kc = pkg.KmerCounter(k)
    kc.submit_reads(*arrays(reads))
    return kc


# ---- chains and circles around the wave, the workgroup and a jumping round, at every key width --------------------------
@pytest.mark.parametrize("k", [21, 31, 32, 33, 77])
def test_chains_and_circles(k):
    rng = np.random.default_rng(5100 + k)
    reads, lengths = [], (1, 2, 3, 64, 65, 4097)
    for i, m in enumerate(lengths):
        reads += cover(chain(rng, m, k), k, times=2 + i % 2)
    circles = ["AC", "ACG"]
    fwd = rev = None
    while fwd is None or rev is None:  # a circle whose smallest k-mer is on the strand the read shows, and one where it is not
        c = rand_seq(rng, 64)
        if smallest_on_forward(c, k):
            fwd = c
        else:
            rev = c
    circles += [fwd, rev, rand_seq(rng, 5000)]
    for c in circles:
        reads += [circle_read(c, k)] * 2
    with counted(k, reads) as kc:
        units, st, R = compare(kc)
        ms = [u[3] for u in units]
        assert len(R) == sum(lengths) + sum(len(c) for c in circles)  # the result set has the shape the reads were built for
        assert sorted(ms) == sorted(lengths + tuple(len(c) for c in circles))
        assert st["circular"] == len(circles) and st["singletons"] == 1 and st["longest"] == 5000 + k - 1
        assert len({u[2] for u in units}) > 1  # depths differ between unitigs (two and three submissions, circles at four)


def test_one_long_chain_beside_many_short_ones():
    k = 21
    rng = np.random.default_rng(5200)
    reads = cover(chain(rng, 270000, k), k)
    for _ in range(2000):
        reads += [chain(rng, int(rng.integers(1, 12)), k)] * 2
    with counted(k, reads) as kc:
        units, st, R = compare(kc)
        assert len(R) > 270000 + 2000 and st["unitigs"] >= 2001
        assert st["longest"] >= (1 << 18) + k  # more than 2^18 k-mers on one path: 19 rounds of jumping or more
        assert st["singletons"] > 50


# ---- the link's conditions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_one_sided_disagreement(k):
    rng = np.random.default_rng(5300 + k)
    strong = rand_seq(rng, 160)
    pos = 70
    y = strong[pos:pos + k]
    d = "ACGT"[("ACGT".index(strong[pos - 1]) + 1) % 4]
    weak = rand_seq(rng, 40) + d + strong[pos:pos + k + 5]
    with counted(k, [strong] * 30 + [weak] * 2) as kc:
        units, st, R = compare(kc)
        yc = M.canonical(y)
        v = d + y[:-1]
        vc = M.canonical(v)
        assert R[yc][0] == 32 and R[vc][0] == 2
        ynode, vnode = (yc, 1 if yc == y else -1), (vc, 1 if vc == v else -1)
        assert M.ext_l(R, ynode) == strong[pos - 1]  # the vote gave the strong branch's base (and no F, or y were purged)
        assert M.ext_r(R, vnode) == y[-1] and M.successor(R, vnode) is None  # v leads to y, y does not agree
        assert any(t.endswith(v) or t.startswith(M.revcomp(v)) for t, _, _, _ in units)


@pytest.mark.parametrize("k", [21, 33])
def test_hairpin_around_a_palindromic_k_minus_1_mer(k):
    rng = np.random.default_rng(5400 + k)
    s = rand_seq(rng, 90)
    read = s + M.revcomp(s)  # the k-mer that ends (k - 1) / 2 bases behind the turn is followed by its own reverse complement
    x = read[90 - (k + 1) // 2:][:k]
    assert read[90 - (k + 1) // 2 + 1:][:k] == M.revcomp(x)
    with counted(k, [read] * 3) as kc:
        units, st, R = compare(kc)
        xc = M.canonical(x)
        assert xc in R
        assert M.successor(R, (xc, 1 if xc == x else -1)) is None
        assert st["unitigs"] == 1 and st["circular"] == 0 and st["longest"] == 90 - 1 + (k - 1) // 2


@pytest.mark.parametrize("k", [22, 32])
def test_palindromic_kmer_at_even_k(k):
    rng = np.random.default_rng(5500 + k)
    h = rand_seq(rng, k // 2)
    p = h + M.revcomp(h)
    read = rand_seq(rng, 60) + p + rand_seq(rng, 60)
    with counted(k, [read] * 2) as kc:
        units, st, R = compare(kc)
        assert p in R and (p, R[p][0], R[p][0], 1) in units
        assert st["unitigs"] == 3 and st["singletons"] == 1


# ---- the smallest sets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32])
def test_empty_and_single_result(k):
    rng = np.random.default_rng(5600 + k)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(*arrays([rand_seq(rng, 100)]))  # every k-mer once: all purged
        g = device_unitigs(kc)
        assert g[0] == b"" and len(g[1]) == 0 and g[2].tolist() == [0] and len(g[3]) == 0
        assert g[4] == dict(kmers=0, unitigs=0, singletons=0, circular=0, bases=0, longest=0)
        assert kc.unitig_strings() == []
        kc.reset()
        one = rand_seq(rng, k + 2)
        kc.submit_reads(*arrays([one] * 2))
        units, st, R = compare(kc)
        assert units == [(M.canonical(one[1:-1]), 2, 2, 1)] and st["kmers"] == 1
        assert kc.unitig_strings() == [(M.canonical(one[1:-1]), 2)]


# ---- the protocol --------------------------------------------------------------------------------------------------------
def small_set(rng, k):
    reads = []
    for m in (1, 5, 40, 300):
        reads += cover(chain(rng, m, k), k)
    reads += [circle_read(rand_seq(rng, 30), k)] * 2
    return reads


def test_capacity_one_short_writes_nothing():
    import torch
    k = 21
    L = pkg.lib()
    with counted(k, small_set(np.random.default_rng(5700), k)) as kc:
        units, st, (seqs, depths, offsets, sums), R = model_of(kc)
        nb, nu = len(seqs), len(units)
        assert nu == 5
        for cap, ucap in ((nb - 1, nu), (nb, nu - 1)):
            d_seqs = torch.full((nb,), 0xAB, dtype=torch.uint8, device="cuda")
            d_dep = torch.full((nb,), 0x5A5A, dtype=torch.int16, device="cuda")
            d_off = torch.full((nu + 1,), -7, dtype=torch.int64, device="cuda")
            d_sum = torch.full((nu,), -9, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            gu, gb, gs = C.c_uint64(0), C.c_uint64(0), _lib.kc_unitig_stats()
            rc = L.kc_build_unitigs(kc._h, d_seqs.data_ptr(), cap, d_dep.data_ptr(), d_off.data_ptr(), ucap, d_sum.data_ptr(), C.byref(gu),
                                    C.byref(gb), C.byref(gs))
            assert rc == _lib.KC_ERR_CAPACITY
            assert (gu.value, gb.value, gs.unitigs, gs.bases) == (nu, nb, nu, nb - nu)  # the totals are filled all the same
            assert (d_seqs.cpu().numpy() == 0xAB).all() and (d_dep.cpu().numpy() == 0x5A5A).all()
            assert (d_off.cpu().numpy() == -7).all() and (d_sum.cpu().numpy() == -9).all()
        compare(kc)  # and the context is as good as before


def test_state_errors():
    k = 21
    L = pkg.lib()
    reads = small_set(np.random.default_rng(5800), k)
    nu, nb = C.c_uint64(5), C.c_uint64(5)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(*arrays(reads))
        assert L.kc_build_unitigs(kc._h, None, 0, None, None, 0, None, C.byref(nu), C.byref(nb), None) == _lib.KC_ERR_STATE  # before finalize
        assert (nu.value, nb.value) == (0, 0)
        compare(kc)  # still usable
    with pkg.KmerCounter(k, rank_me=0, rank_n=2) as kc:
        kc.submit_reads(*arrays(reads))
        kc.finalize()
        assert L.kc_build_unitigs(kc._h, None, 0, None, None, 0, None, C.byref(nu), C.byref(nb), None) == _lib.KC_ERR_STATE
        assert b"across shards" in L.kc_last_error()


@pytest.mark.parametrize("k", [21, 31])
def test_twice_the_same_and_the_other_consumers_undisturbed(k):
    rng = np.random.default_rng(5900 + k)
    reads = small_set(rng, k)
    with counted(k, reads) as kc, counted(k, reads) as plain:
        keys, counts, left, right = kc.results()  # unsorted yet
        queries = np.concatenate([keys, np.array([[int(v) for v in rng.integers(0, 1 << 62, size=kc.nl)] for _ in range(200)],
                                                 dtype=np.uint64).reshape(-1, kc.nl)])
        before = kc.lookup(queries)
        assert (before[0][:len(counts)] == counts).all()
        text = plain.dump_text()
        first = device_unitigs(kc)
        second = device_unitigs(kc)
        assert first[0] == second[0] and first[4] == second[4]
        for a, b in zip(first[1:4], second[1:4]):
            assert (a == b).all()
        # without the optional arrays: the same block and offsets
        bare = device_unitigs(kc, depths=False, sums=False)
        assert bare[0] == first[0] and (bare[2] == first[2]).all()
        only_depths = device_unitigs(kc, depths=True, sums=False)
        assert (only_depths[1] == first[1]).all()
        after = kc.lookup(queries)
        for a, b in zip(after, before):
            assert (a == b).all()
        assert kc.dump_text() == text
        # the Python wrappers
        seqs, offsets, sums, st = kc.unitigs()
        assert seqs.cpu().numpy().tobytes() == first[0] and (offsets.cpu().numpy().astype(np.uint64) == first[2]).all()
        assert (sums.cpu().numpy().astype(np.uint64) == first[3]).all() and st == first[4]
        blk, dep = kc.unitig_block()
        assert blk.cpu().numpy().tobytes() == first[0] and (dep.cpu().numpy().view(np.uint16) == first[1]).all()
        units = M.unitigs(M.results_dict(*plain.results(), k), k)[0]
        assert kc.unitig_strings() == [(t, s) for t, s, _, _ in units]
        times = None
    with pkg.KmerCounter(k, time_kernels=True) as kc:
        kc.submit_reads(*arrays(reads))
        kc.unitigs()
        times = kc.kernel_times()
        n2 = 2 * len(counts)
        rounds = (n2 - 1).bit_length() + 1
        assert times["kc_unitig_min_jump_kernel"][0] == 2 * rounds and times["kc_unitig_rank_jump_kernel"][0] == 2 * rounds  # query + call
        for name in ("links", "cut", "select", "scan"):
            assert times["kc_unitig_%s_kernel" % name][0] == 2
        assert times["kc_unitig_write_kernel"][0] == 1 and "kc_unitig_depth_kernel" not in times


# ---- the loop: k = 21 -> unitigs -> k = 33 with contig k-mers --------------------------------------------------------------
def test_unitigs_feed_the_next_k_through_the_device_contig_path():
    rng = np.random.default_rng(6000)
    reads = []
    for g in range(6):  # six genomes at different coverage: six or more unitigs of different depths
        genome = rand_seq(rng, 500)
        for _ in range(60 + 40 * g):
            a = int(rng.integers(0, len(genome) - 160))
            r = genome[a:a + int(rng.integers(40, 150))]
            reads.append(r if rng.random() < 0.5 else M.revcomp(r))
    b, q, offs = arrays(reads)
    with pkg.KmerCounter(21) as kc, pkg.KmerCounter(21) as host:
        kc.submit_reads(b, q, offs)
        host.submit_reads(b, q, offs)
        units = M.unitigs(M.results_dict(*host.results(), 21), 21)[0]
        assert len(units) >= 6 and max(u[3] for u in units) > 200 and len({u[2] for u in units}) >= 4
        seqs, depths = kc.unitig_block()
        kc.reset(33)
        kc.submit_reads(b, q, offs)
        kc.begin_ctg_kmers(seqs.numel())
        kc.submit_ctg_block(seqs, depths)
        got = kc.sorted_results()
        host.reset(33)
        host.submit_reads(b, q, offs)
        host.begin_ctg_kmers(sum(len(u[0]) + 1 for u in units))
        host.submit_ctgs([u[0] for u in units], [u[2] for u in units])
        want = host.sorted_results()
        assert kc.ctg_stats() == host.ctg_stats()
        assert len(want[1]) > 1000
        for g, w, name in zip(got, want, ("keys", "counts", "left", "right")):
            assert g.shape == w.shape and (g == w).all(), name
