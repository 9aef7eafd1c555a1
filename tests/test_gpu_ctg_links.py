"""kc_ctg_links (csrc/kc_links.hpp) against the host model tests/links_model.py, byte for byte: the records, end_first and
the statistics on the same inputs.  The model is never replaced by a second device run.

Every device call goes through device_links: offsets, records, pairs, links and end_first in device arrays of exactly
their size, the record arrays inside canaries.  The call reads no base, so the records are forged (the chain test at the
end excepted): a supporter of a link is a read of 64 bases with ten of them at the end of one contig and ten at the start
of another, or a pair with a mate on each."""
import ctypes as C

import numpy as np
import pytest

import depth_model as D
import links_cases as LC
import links_model as M
import mhm2_kmer_analysis_v2_amd as pkg
import test_links_model as T
from depth_model import NO_ALN, PAIR_DTYPE, rec, records
from mhm2_kmer_analysis_v2_amd import _lib
from test_gpu_aln_depths import NONE_REC, PAD, lengths_index, rand_seq
from test_gpu_gap_align import block_arrays, read_arrays

pytestmark = pytest.mark.gpu

SORT_TILE = 4096  # kc_sort.hpp: items (two a candidate) a workgroup and pass
CL, RL, PIECE = 30, 64, 10  # forged cases: every contig's length, every read's, and the bases a read has on a contig
BIG = (1 << 15) + 1  # contigs of the shared index: an end's number takes 17 bits, two whole digits of the sort and one bit


def stats_dict(st):
    return {n: int(getattr(st, n)) for n in M.LINK_STATS}


UNTOUCHED = dict(dict.fromkeys(M.LINK_STATS, 0), reads=99)


def offsets_of(read_lens):
    offs = np.zeros(len(read_lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.asarray(read_lens, dtype=np.uint64))
    return offs


def canaried(raw, shift=0, fill=0xCD):
    """a device byte array with raw at PAD + shift between canaries, and its host image"""
    import torch
    h = np.full(len(raw) + 2 * PAD + 16, fill, dtype=np.uint8)
    h[PAD + shift:PAD + shift + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return torch.from_numpy(h).cuda(), h


def device_links(kc, n_ctgs, read_lens, alns, pairs=None, n=0, expect=0, shift=0, capacity=None, want_links=True, want_ef=True,
                 want_stats=True, **kw):
    """the call on device arrays of exactly the needed size (n records) inside canaries: (links, end_first, stats).
    expect != 0: the status is checked, and that nothing was written but, for KC_ERR_CAPACITY, the count and the
    statistics; shift: bytes by which the record arrays are misaligned; capacity: by default n."""
    import torch
    nreads, na, n_ef = len(read_lens), len(alns), 2 * n_ctgs + 1
    d_in, h_in = canaried(alns.tobytes(), shift)
    d_pr, h_pr = canaried(pairs.tobytes() if pairs is not None else b"", shift)
    d_o = torch.from_numpy(offsets_of(read_lens).view(np.int64)).cuda()
    d_links = torch.full((n * 48 + 2 * PAD + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ef = torch.full((n_ef * 8 + 2 * PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st, cnt = _lib.kc_link_stats(reads=99), C.c_uint64(0xABAB)
    p = _lib.kc_link_params(**M.params(**kw))
    rc = pkg.lib().kc_ctg_links(kc._h, d_o.data_ptr(), nreads, d_in.data_ptr() + PAD + shift, na,
                                d_pr.data_ptr() + PAD + shift if pairs is not None else None, 1, C.byref(p),
                                d_links.data_ptr() + PAD + shift if want_links else None, n if capacity is None else capacity,
                                d_ef.data_ptr() + PAD if want_ef else None, C.byref(cnt), C.byref(st) if want_stats else None)
    h_links, h_ef = d_links.cpu().numpy(), d_ef.cpu().numpy()
    assert (d_in.cpu().numpy() == h_in).all() and (d_pr.cpu().numpy() == h_pr).all(), "the input records were written"
    if expect:
        assert rc == expect, (rc, pkg.lib().kc_last_error())
        assert (h_links == 0xAB).all() and (h_ef == 0xAB).all(), "a refused call wrote"
        if expect == _lib.KC_ERR_CAPACITY:
            return int(cnt.value), stats_dict(st)
        assert stats_dict(st) == UNTOUCHED and cnt.value == 0xABAB, "a refused call wrote the count or the statistics"
        return rc
    assert rc == 0, pkg.lib().kc_last_error()
    assert (h_links[:PAD + shift] == 0xAB).all() and (h_links[PAD + shift + n * 48:] == 0xAB).all(), "a canary was written"
    assert (h_ef[:PAD] == 0xAB).all() and (h_ef[PAD + n_ef * 8:] == 0xAB).all(), "a canary was written"
    if not want_links:
        assert (h_links == 0xAB).all()
    if not want_ef:
        assert (h_ef == 0xAB).all()
    if not want_stats:
        assert stats_dict(st) == UNTOUCHED
    assert cnt.value == n or not want_links, (cnt.value, n)
    return (h_links[PAD + shift:PAD + shift + n * 48].copy().view(M.LINK_DTYPE), h_ef[PAD:PAD + n_ef * 8].copy().view(np.uint64), stats_dict(st),
            int(cnt.value))


def same(got, want):
    assert got[2] == want[2]
    if got[0].tobytes() != want[0].tobytes():
        diff = [j for j in range(len(want[0])) if got[0][j].tobytes() != want[0][j].tobytes()]
        assert not diff, (diff[:5], got[0][diff[:5]], want[0][diff[:5]])
    assert (got[1] == want[1]).all(), np.nonzero(got[1] != want[1])[0][:8]


def compare(kc, ctg_lens, read_lens, alns, pairs=None, **kw):
    want = M.ctg_links(ctg_lens, read_lens, alns, pairs, **kw)
    same(device_links(kc, len(ctg_lens), read_lens, alns, pairs, n=len(want[0]), **kw), want)
    return want


# ---- forged supporters, as arrays -----------------------------------------------------------------------------------------
def gap_records(read, ctg, cstart, cstop, rstart, rstop, orient):
    out = np.zeros(len(read), dtype=M.GAP_ALN_DTYPE)
    for n, v in (("read", read), ("ctg", ctg), ("cstart", cstart), ("cstop", cstop), ("rstart", rstart), ("rstop", rstop), ("orient", orient)):
        out[n] = v
    out["score"] = 2 * (out["cstop"] - out["cstart"])
    out["seeds"] = 1
    return out


def splints(read, u, v, gap, oa=0, ob=0, ea=0, eb=0):
    """two records a read (arrays, one entry a read): PIECE bases that leave contig u, ea from its end, then, gap read
    bases on, PIECE bases that enter contig v, eb from its end; oa / ob the pieces' orientations"""
    read, u, v, gap, oa, ob, ea, eb = (np.broadcast_to(np.asarray(x, dtype=np.int64), np.shape(read)) for x in (read, u, v, gap, oa, ob, ea, eb))
    qa, qb = np.full(read.shape, 20), 20 + PIECE + gap  # the pieces' first read bases: room for an overlap in front
    a_c = np.where(oa == 0, CL - ea - PIECE, ea)  # it leaves through the right end iff it lies forward
    b_c = np.where(ob == 0, eb, CL - eb - PIECE)
    a_r, b_r = np.where(oa == 0, qa, RL - qa - PIECE), np.where(ob == 0, qb, RL - qb - PIECE)
    a = gap_records(read, u, a_c, a_c + PIECE, a_r, a_r + PIECE, oa)
    b = gap_records(read, v, b_c, b_c + PIECE, b_r, b_r + PIECE, ob)
    return np.stack([a, b], axis=1).reshape(-1)


def spans(first_read, first_aln, u, v, d0, d1, cl=CL):
    """(records, pairs): pair i has mate 2i forward on contig u, its first base d0 from u's right end, and mate 2i + 1
    reversed on contig v, its first base d1 from v's left end (the mates hang over the contigs' far ends where d exceeds
    the contig, which d below cl + RL allows); the pairs name them"""
    u, v, d0, d1 = (np.asarray(x, dtype=np.int64) for x in np.broadcast_arrays(u, v, d0, d1))
    i = np.arange(len(u))
    s0 = cl - d0  # where mate 2i begins on u: below 0 it is clipped
    c0, c1 = np.maximum(s0, 0), np.minimum(s0 + RL, cl)
    a = gap_records(first_read + 2 * i, u, c0, c1, c0 - s0, c1 - s0, 0)
    t0 = d1 - RL  # mate 2i + 1 in contig orientation covers [d1 - RL, d1) of v
    e0, e1 = np.maximum(t0, 0), np.minimum(d1, cl)
    b = gap_records(first_read + 2 * i + 1, v, e0, e1, e0 - t0, e1 - t0, 1)
    pairs = np.zeros(len(u), dtype=PAIR_DTYPE)
    pairs["aln0"], pairs["aln1"] = first_aln + 2 * i, first_aln + 2 * i + 1
    return np.stack([a, b], axis=1).reshape(-1), pairs


def no_pairs(n):
    out = np.zeros(n, dtype=PAIR_DTYPE)
    out["aln0"] = out["aln1"] = NO_ALN
    return out


@pytest.fixture(scope="module")
def big():
    """one index of BIG contigs of CL bases for the forged cases"""
    with lengths_index([CL] * BIG, time_kernels=True) as kc:
        yield kc


LENS = T.LENS


@pytest.fixture(scope="module")
def small():
    with lengths_index(LENS) as kc:
        yield kc


# ---- the model's cases --------------------------------------------------------------------------------------------------
def test_the_models_splint_cases(small):
    kc, L = small, 100
    for gap in (0, 7, -20):
        for oa, ob in ((0, 0), (0, 1), (1, 0), (1, 1)):
            alns = records([T.leaving(0, L, 0, 50, 0, LENS[0], oa), T.entering(0, L, 50 + gap, L, 1, LENS[1], ob)])
            w = compare(kc, LENS, [L, 0], alns)
            assert len(w[0]) == 2 and int(w[0][0]["splint_gap_sum"]) == gap
            compare(kc, LENS, [L, 0], alns[::-1].copy())
    for ea, eb in ((5, 0), (6, 0), (0, 5), (0, 6), (5, 5), (6, 6)):
        alns = records([T.leaving(0, L, 0, 50, 0, LENS[0], 0, e=ea), T.entering(0, L, 53, L, 1, LENS[1], 0, e=eb)])
        assert len(compare(kc, LENS, [L, 0], alns, end_slack=5)[0]) == (2 if max(ea, eb) == 5 else 0)
    alns = records([T.leaving(0, L, 0, 50, 0, LENS[0], 1, e=1), T.entering(0, L, 50, L, 1, LENS[1], 1)])
    assert [len(compare(kc, LENS, [L, 0], alns, end_slack=s)[0]) for s in (0, 1, 1024)] == [0, 2, 2]
    for gap in (30, 31, -40, -41):
        alns = records([T.leaving(0, 200, 0, 100, 0, LENS[0], 0), T.entering(0, 200, 100 + gap, 200, 1, LENS[1], 1)])
        w = compare(kc, LENS, [200, 0], alns, max_overlap=40, max_splint_gap=30)
        assert w[2]["splint_cands"] + w[2]["splints_gap_out"] == 1 and w[2]["splint_cands"] == (gap in (30, -40))
    # equal starts, equal stops, two records on one contig, records of kind NONE and filtered records
    for alns in (records([T.leaving(0, L, 10, 50, 0, LENS[0], 0), T.entering(0, L, 10, 60, 1, LENS[1], 0)]),
                 records([T.leaving(0, L, 10, 60, 0, LENS[0], 0), T.entering(0, L, 20, 60, 1, LENS[1], 0)]),
                 records([T.leaving(0, L, 0, 50, 0, LENS[0], 0), T.entering(0, L, 50, L, 0, LENS[0], 0), NONE_REC])):
        assert len(compare(kc, LENS, [L, 0], alns)[0]) == 0
    alns = records([T.leaving(0, L, 0, 50, 0, LENS[0], 0, score=99), NONE_REC, T.entering(0, L, 50, L, 1, LENS[1], 0, score=100), NONE_REC])
    assert [compare(kc, LENS, [L, 0], alns, min_score=s)[2]["filtered"] for s in (99, 100, 101)] == [0, 1, 2]
    assert [compare(kc, LENS, [L, 0], alns, min_len=s)[2]["links"] for s in (50, 51)] == [1, 0]


def test_the_models_three_contigs_and_the_cap():
    L, mid = 300, 60
    lens = [300, mid, 250]
    alns = records([T.leaving(0, L, 0, 100, 0, lens[0], 0), rec(0, 1, 0, mid, rstart=100, rstop=160), T.entering(0, L, 160, L, 2, lens[2], 0)])
    with lengths_index(lens) as kc:
        assert len(compare(kc, lens, [L, 0], alns, max_splint_gap=59)[0]) == 4
        assert len(compare(kc, lens, [L, 0], alns, max_splint_gap=60)[0]) == 6
    # reads with 0, 1, 2, max_read_alns and max_read_alns + 1 passing records, each a chain of whole contigs
    for cap in (2, 64):
        lens = [12] * (cap + 1)
        rows, counts = [], (0, 1, 2, cap, cap + 1, cap)
        for r, c in enumerate(counts):
            rows += [rec(r, u, 0, 12, rstart=15 * u, rstop=15 * u + 12) for u in range(c)]
        rows.append(rec(5, cap, 0, 12, rstart=15 * cap, rstop=15 * cap + 12, score=1))  # read 5: one more, but it does not pass
        with lengths_index(lens) as kc:
            w = compare(kc, lens, [1024] * len(counts), records(rows), max_read_alns=cap, max_splint_gap=3, min_score=2)
            assert w[2]["reads_over_cap"] == 1 and w[2]["filtered"] == 1
            assert w[2]["splint_cands"] == 1 + 2 * (cap - 1) and w[2]["links"] == cap - 1
            rng = np.random.default_rng(cap)
            compare(kc, lens, [1024] * len(counts), records(rows)[rng.permutation(len(rows))], max_read_alns=cap, max_splint_gap=3, min_score=2)


def test_the_models_span_cases():
    lens, f = [1000, 800], 700
    with lengths_index(lens) as kc:
        for o0, o1 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            for gap in (0, 25, -30):
                alns, pairs = T.span_case(o0, o1, gap, f)
                w = compare(kc, lens, [100, 100], alns, pairs, insert_avg=f, max_insert=900)
                assert len(w[0]) == 2 and int(w[0][0]["span_gap_sum"]) == gap
                assert compare(kc, lens, [100, 100], alns, pairs, insert_avg=f - gap, max_insert=f - gap)[2]["span_cands"] == 1
                assert compare(kc, lens, [100, 100], alns, pairs, insert_avg=f - gap - 1, max_insert=f - gap - 1)[2]["spans_too_far"] == 1
                compare(kc, lens, [100, 100], alns, None, insert_avg=f)
        for x in ((NO_ALN, 1), (0, NO_ALN), (NO_ALN, NO_ALN)):
            q = pairs.copy()
            q[0]["aln0"], q[0]["aln1"] = x
            compare(kc, lens, [100, 100], alns, q, insert_avg=f)
        # a splint and a span on one link
        L = 100
        alns, pairs = T.span_case(0, 0, 12, 700)
        splint = [T.leaving(2, L, 0, 40, 0, lens[0], 0), T.entering(2, L, 52, L, 1, lens[1], 0)]
        alns = records(list(alns) + splint + splint)
        w = compare(kc, lens, [L] * 4, alns, np.concatenate([pairs, no_pairs(1)]), insert_avg=700)
        assert w[2]["links_both"] == 1 and (int(w[0][0]["splints"]), int(w[0][0]["spans"])) == (4, 1)
    lens = [200, 800]  # a mate hanging over its contig's far end
    alns = records([rec(0, 0, 0, 90, rstart=10, rstop=100), rec(1, 1, 100, 190, rstart=0, rstop=90, orient=1)])
    with lengths_index(lens) as kc:
        compare(kc, lens, [100, 100], alns, pairs, insert_avg=500, max_insert=500)


@pytest.mark.parametrize("seed", [1, 2])
def test_the_models_mirrors_and_shuffles(seed):
    rng = np.random.default_rng(seed)
    lens, read_lens, alns, pairs = T.random_case(rng)
    kw = dict(end_slack=5, max_overlap=15, max_splint_gap=12, insert_avg=300, max_insert=500)
    with lengths_index(lens) as kc:
        compare(kc, lens, read_lens, alns, pairs, **kw)
        plain = compare(kc, lens, read_lens, alns, None, **kw)
        perm = rng.permutation(len(alns))
        same(device_links(kc, len(lens), read_lens, alns[perm], None, n=len(plain[0]), **kw), plain)  # in read order and shuffled: one output
        compare(kc, lens, read_lens, T.revcomp_reads(alns, list(range(0, len(read_lens), 3))), None, **kw)
        compare(kc, lens, read_lens, T.flip_contig(alns, 3, lens[3], read_lens), pairs, **kw)


# ---- sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, SORT_TILE // 2 - 1, SORT_TILE // 2, SORT_TILE // 2 + 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1,
                               3 * SORT_TILE + 1])
def test_candidate_totals_around_the_sorts_tile(big, n):
    """n candidates are 2 n sorted items: the tile's edge in items and in candidates.  Two thirds are splints over
    random links among 700 contigs (runs of several supporters), the rest spans."""
    rng = np.random.default_rng(n)
    ns = n - n // 3
    u = rng.integers(0, 700, size=n)
    v = (u + rng.integers(1, 700, size=n)) % 700
    a = splints(np.arange(ns), u[:ns], v[:ns], rng.integers(-9, 9, size=ns), rng.integers(0, 2, size=ns), rng.integers(0, 2, size=ns),
                rng.integers(0, 3, size=ns), rng.integers(0, 3, size=ns))
    first_read = ns + (ns & 1)
    b, pairs = spans(first_read, 2 * ns, u[ns:], v[ns:], rng.integers(1, 90, size=n - ns), rng.integers(1, 90, size=n - ns))
    alns = np.concatenate([a, b])
    pairs = np.concatenate([no_pairs(first_read // 2), pairs])
    nreads = first_read + 2 * (n - ns)
    w = compare(big, [CL] * BIG, [RL] * nreads, alns, pairs, end_slack=2, max_overlap=20, max_splint_gap=20, insert_avg=300, max_insert=1000)
    assert w[2]["splint_cands"] + w[2]["span_cands"] == n and w[2]["splints_gap_out"] == w[2]["spans_too_far"] == 0


def test_runs_of_one_to_seventy_thousand_supporters_and_sums_past_32_bits(big):
    """links with 1, 63, 64, 65, 4097 and 70 000 supporters beside 5000 links of one supporter each: a run inside a wave,
    across waves, across the reduce kernel's tiles and across the sort's.  The 70 000 are spans at gap 65 533: their sum
    needs 33 bits.  The splints' gaps are all negative: so are their minima and maxima."""
    rng = np.random.default_rng(5)
    sizes = (1, 63, 64, 65)
    u = np.concatenate([np.full(s, 10 + 2 * i) for i, s in enumerate(sizes)] + [np.arange(1000, 6000)])
    ns = len(u)
    a = splints(np.arange(ns), u, u + 1, rng.integers(-9, -3, size=ns), 0, (u // 2) % 2)  # into end 2 (u + 1) or 2 (u + 1) + 1
    first_read, nb, nc = ns + (ns & 1), 70000, 4097
    b, pb = spans(first_read, 2 * ns, np.full(nb, 100), 200, 1, 1)  # gap = insert_avg - 1 - 1
    c, pc = spans(first_read + 2 * nb, 2 * ns + 2 * nb, np.full(nc, 300), 301, rng.integers(1, 90, size=nc), rng.integers(1, 90, size=nc))
    alns = np.concatenate([a, b, c])
    nreads = first_read + 2 * nb + 2 * nc
    pairs = np.concatenate([no_pairs(first_read // 2), pb, pc])
    w = compare(big, [CL] * BIG, [RL] * nreads, alns, pairs, max_overlap=20, max_splint_gap=20, insert_avg=65535, max_insert=65535)
    x = {(int(r["from"]), int(r["to"])): r for r in w[0]}
    assert int(x[(201, 400)]["spans"]) == nb and int(x[(201, 400)]["span_gap_sum"]) == nb * 65533 > 1 << 32
    assert int(x[(601, 602)]["spans"]) == nc and int(x[(601, 602)]["span_gap_min"]) < int(x[(601, 602)]["span_gap_max"])
    assert [int(x[e]["splints"]) for e in ((21, 23), (25, 26), (29, 31), (33, 34))] == list(sizes)
    assert all(int(r["splint_gap_max"]) < 0 for r in w[0] if r["splints"])
    assert (w[2]["splint_cands"], w[2]["span_cands"], w[2]["links"], w[2]["links_both"]) == (ns, nb + nc, 4 + 5000 + 2, 0)


def test_span_gaps_that_sum_below_minus_two_to_the_31():
    """33 000 pairs over one link at gaps of about -65 530: the sum is below -2^31, the minimum and the maximum negative"""
    cl, n = 32800, 33000
    i = np.arange(n)
    alns, pairs = spans(0, 0, np.zeros(n), 1, 32767 - i % 3, 32768 - i % 5, cl=cl)
    with lengths_index([cl, cl]) as kc:
        w = compare(kc, [cl, cl], [RL] * (2 * n), alns, pairs, insert_avg=1, max_insert=65535)
        x = w[0][0]
        assert (int(x["from"]), int(x["to"]), int(x["spans"])) == (1, 2, n) and int(x["span_gap_sum"]) < -(1 << 31)
        assert (int(x["span_gap_min"]), int(x["span_gap_max"])) == (-65534, -65528)
        assert compare(kc, [cl, cl], [RL] * (2 * n), alns, pairs, insert_avg=1, max_insert=65534)[2]["spans_too_far"] == (n + 14) // 15


def test_a_hub_the_last_end_and_two_contigs(big):
    """end 3 linked to 3000 other ends: a long row of end_first among empty ones, the first and the last end empty; and
    links to the last end of all, whose number has bit 16 set"""
    n = 3000
    a = splints(np.arange(n), 1, np.arange(2, n + 2), 0)
    w = compare(big, [CL] * BIG, [RL] * n, a)
    ef = [int(x) for x in w[1]]
    assert ef[:5] == [0, 0, 0, 0, n] and ef[5] == n + 1 and ef[-1] == 2 * n and ef[2 * n + 5:] == [2 * n] * (2 * BIG + 1 - 2 * n - 5)
    assert w[2]["ends_linked"] == n + 1
    last = BIG - 1
    a = np.concatenate([splints(np.arange(4), [0, 5, last, last - 1], [last, last, 7, last], [1, 2, 3, 4], 0, [1, 1, 0, 1]),
                        splints(np.arange(4, 6), [0, 1], [1, 0], 0, 1, [0, 1])])
    w = compare(big, [CL] * BIG, [RL] * 6, a)
    assert int(w[0][-1]["from"]) == 2 * BIG - 1 and int(w[1][-2]) < int(w[1][-1]) == len(w[0]) == 12
    with lengths_index([CL, CL]) as kc:  # two contigs: one bit an end... two
        for oa in (0, 1):
            for ob in (0, 1):
                a = np.concatenate([splints(np.arange(3), 0, 1, [1, 2, 3], oa, ob), splints(np.arange(3, 5), 1, 0, [4, 5], ob ^ 1, oa ^ 1)])
                w = compare(kc, [CL, CL], [RL] * 6, a)
                assert len(w[0]) == 2 and int(w[0][0]["splints"]) == 5 and int(w[0][0]["splint_gap_sum"]) == 15


# ---- the protocol -------------------------------------------------------------------------------------------------------
def small_case():
    """three contigs, eight reads: a splint 1 -- 2 twice, a splint 3 -- 5 into a reversed piece, a span 1 -- 2 and one too far"""
    L = 100
    rows = [T.leaving(0, L, 0, 50, 0, LENS[0], 0), T.entering(0, L, 57, L, 1, LENS[1], 0),
            T.leaving(1, L, 5, 50, 0, LENS[0], 0, e=2), T.entering(1, L, 48, L, 1, LENS[1], 0, e=1), NONE_REC,
            T.leaving(3, L, 0, 40, 1, LENS[1], 0), T.entering(3, L, 41, 90, 2, LENS[2], 1),
            rec(4, 0, 100, 200), rec(5, 1, 150, 250, orient=1), rec(6, 0, 0, 100), rec(7, 2, 101, 201, orient=1)]
    pairs = np.zeros(4, dtype=PAIR_DTYPE)
    pairs[:] = [(0, 2, 0, 0, (0, 0, 0)), (NO_ALN, 5, 0, 0, (0, 0, 0)), (7, 8, 0, 0, (0, 0, 0)), (9, 10, 0, 0, (0, 0, 0))]
    return [L] * 8, records(rows), pairs


KW = dict(insert_avg=460, max_insert=500)


def test_optional_outputs_capacity_host_arrays_and_the_wrapper():
    import torch
    read_lens, alns, pairs = small_case()
    want = M.ctg_links(LENS, read_lens, alns, pairs, **KW)
    assert [(int(x["from"]), int(x["to"]), int(x["splints"]), int(x["spans"])) for x in want[0]] == [(1, 2, 2, 1), (2, 1, 2, 1), (3, 5, 1, 0), (5, 3, 1, 0)]
    assert (want[2]["spans_too_far"], want[2]["none"], int(want[0][0]["span_gap_sum"]), int(want[0][0]["splint_gap_sum"])) == (1, 1, 10, 2)
    n = len(want[0])
    with lengths_index(LENS, time_kernels=True) as kc:
        kc.kernel_times(clear=True)
        compare(kc, LENS, read_lens, alns, pairs, **KW)
        times = {k: v[0] for k, v in kc.kernel_times(clear=True).items()}
        assert times == {"kc_align_lengths_kernel<links>": 1, "kc_depth_check_kernel<links>": 1, "kc_lassm_pair_check_kernel<links>": 1,
                         "kc_link_group_kernel<count>": 1, "kc_link_group_kernel<fill>": 1, "kc_link_tile_scan_kernel": 2, "kc_link_scan_kernel": 3,
                         "kc_link_cands_kernel<count>": 1, "kc_link_cands_kernel<write>": 1, "kc_sort_hist_kernel<links>": 2,
                         "kc_sort_scan_kernel<links>": 2, "kc_sort_scatter_kernel<links>": 2, "kc_link_heads_kernel": 1,
                         "kc_link_reduce_kernel": 1, "kc_link_emit_kernel": 1, "kc_link_end_first_kernel": 1}
        # pairs NULL: no spans, and no pair check
        w = compare(kc, LENS, read_lens, alns, None, **KW)
        assert w[2]["span_cands"] == w[2]["spans_too_far"] == 0 and "kc_lassm_pair_check_kernel<links>" not in kc.kernel_times(clear=True)
        # end_first and stats NULL in turn
        got = device_links(kc, 3, read_lens, alns, pairs, n=n, want_ef=False, **KW)
        assert got[0].tobytes() == want[0].tobytes() and got[2] == want[2]
        got = device_links(kc, 3, read_lens, alns, pairs, n=n, want_stats=False, **KW)
        assert got[0].tobytes() == want[0].tobytes() and (got[1] == want[1]).all()
        # links NULL: a size query; a capacity one under: the count and the statistics and nothing else; more than enough
        got = device_links(kc, 3, read_lens, alns, pairs, n=n, want_links=False, want_ef=False, **KW)
        assert got[3] == n and got[2] == want[2]
        got = device_links(kc, 3, read_lens, alns, pairs, n=n, want_links=False, **KW)  # end_first is not written by a size query
        assert (got[1] == 0xABABABABABABABAB).all()
        assert device_links(kc, 3, read_lens, alns, pairs, n=n, capacity=n - 1, expect=_lib.KC_ERR_CAPACITY, **KW) == (n, want[2])
        assert b"kc_ctg_links: 4 records, the array holds 3" in pkg.lib().kc_last_error()
        assert device_links(kc, 3, read_lens, alns, pairs, n=n, capacity=0, expect=_lib.KC_ERR_CAPACITY, **KW) == (n, want[2])
        same(device_links(kc, 3, read_lens, alns, pairs, n=n, capacity=1 << 40, **KW), want)
        # no records: KC_OK, no links, an all-zero end_first; and no reads
        w = compare(kc, LENS, read_lens, records([]), no_pairs(4), **KW)
        assert len(w[0]) == 0 and not w[1].any() and w[2]["reads"] == 8
        compare(kc, LENS, [], records([]), None, **KW)
        compare(kc, LENS, [], records([]), no_pairs(0), **KW)
        # host arrays, inside canaries of their own
        offs = offsets_of(read_lens)
        h_links = np.full((n + 2) * 48, 0xAB, dtype=np.uint8)
        h_ef = np.full(7 + 2, 0xABABABABABABABAB, dtype=np.uint64)
        st, cnt = _lib.kc_link_stats(), C.c_uint64(0)
        p = _lib.kc_link_params(**M.params(**KW))
        for rep in range(2):  # called twice
            rc = pkg.lib().kc_ctg_links(kc._h, offs.ctypes.data, 8, alns.ctypes.data, len(alns), pairs.ctypes.data, 0, C.byref(p),
                                        h_links.ctypes.data + 48, n, h_ef.ctypes.data + 8, C.byref(cnt), C.byref(st))
            assert rc == 0 and stats_dict(st) == want[2] and cnt.value == n
            assert h_links[48:-48].tobytes() == want[0].tobytes() and h_ef[1:-1].tobytes() == want[1].tobytes()
            assert (h_links[:48] == 0xAB).all() and (h_links[-48:] == 0xAB).all() and h_ef[0] == h_ef[-1] == 0xABABABABABABABAB
        rc = pkg.lib().kc_ctg_links(kc._h, offs.ctypes.data, 8, alns.ctypes.data, len(alns), pairs.ctypes.data, 0, C.byref(p), None, 0, None,
                                    C.byref(cnt), None)
        assert rc == 0 and cnt.value == n
        # the wrapper, both modes, twice
        for rep in range(2):
            links, ef, st, gap = kc.ctg_links(offs, alns, pairs, **KW)
            assert links.dtype == M.LINK_DTYPE and ef.dtype == np.uint64 and (links.tobytes(), ef.tobytes(), st) == (want[0].tobytes(), want[1].tobytes(), want[2])
            assert gap.dtype == np.float64 and (gap == M.mean_gap(want[0])).all() and list(gap) == [1.0, 1.0, 1.0, 1.0]
        w2 = M.ctg_links(LENS, read_lens, alns, None, end_slack=0, **KW)
        d_alns = torch.from_numpy(np.frombuffer(alns.tobytes(), dtype=np.uint8).copy()).cuda()
        d_pairs = torch.from_numpy(np.frombuffer(pairs.tobytes(), dtype=np.uint8).copy()).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        links, ef, st, gap = kc.ctg_links(d_offs, d_alns, None, end_slack=0, **KW)
        assert links.is_cuda and ef.is_cuda and (links.cpu().numpy().tobytes(), ef.cpu().numpy().tobytes(), st) == (w2[0].tobytes(), w2[1].tobytes(), w2[2])
        links, ef, st, gap = kc.ctg_links(d_offs, d_alns, d_pairs, **KW)
        assert (links.cpu().numpy().tobytes(), ef.cpu().numpy().tobytes(), st) == (want[0].tobytes(), want[1].tobytes(), want[2])
        assert (gap == M.mean_gap(want[0])).all()
        links, ef, st, gap = kc.ctg_links(offs, alns[:0], None)
        assert len(links) == 0 and len(gap) == 0 and not ef.any() and st["links"] == 0


def test_names_and_launch_counts_in_the_kernel_times():
    read_lens, alns, pairs = small_case()  # splints and a span: the sort passes and the reduce kernel run
    with lengths_index(LENS, time_kernels=True) as kc:
        kc.kernel_times(clear=True)
        links, _, st, _ = kc.ctg_links(offsets_of(read_lens), alns, pairs, **KW)
        assert len(links) == 4 and st["span_cands"] > 0
        t = kc.kernel_times()
    # an end's number takes 3 bits: one radix pass a word
    want = {"kc_align_lengths_kernel<links>": 1, "kc_depth_check_kernel<links>": 1, "kc_lassm_pair_check_kernel<links>": 1,
            "kc_link_group_kernel<count>": 1, "kc_link_group_kernel<fill>": 1, "kc_link_tile_scan_kernel": 2, "kc_link_scan_kernel": 3,
            "kc_link_cands_kernel<count>": 1, "kc_link_cands_kernel<write>": 1, "kc_sort_hist_kernel<links>": 2,
            "kc_sort_scan_kernel<links>": 2, "kc_sort_scatter_kernel<links>": 2, "kc_link_heads_kernel": 1, "kc_link_reduce_kernel": 1,
            "kc_link_emit_kernel": 1, "kc_link_end_first_kernel": 1}
    assert {n: c for n, (c, _) in t.items()} == want


def test_the_wrapper_calls_once_more_when_four_a_contig_are_too_few():
    lens = [CL] * 12  # room for 4 * 12 + 16 = 64 records; every end linked to every end of the other contigs wants 12 * 11 * 2 * 2
    rows, r = [], 0
    for u in range(12):
        for v in range(12):
            if u != v:
                rows += [splints(np.array([r]), u, v, 1, 0, 0), splints(np.array([r + 1]), u, v, 1, 0, 1)]
                r += 2
    alns = np.concatenate(rows)
    with lengths_index(lens) as kc:
        w = M.ctg_links(lens, [RL] * r, alns)
        assert len(w[0]) > 4 * 12 + 16
        links, ef, st, gap = kc.ctg_links(offsets_of([RL] * r), alns)
        assert (links.tobytes(), ef.tobytes(), st) == (w[0].tobytes(), w[1].tobytes(), w[2]) and len(gap) == len(links)


def test_invalid_reads_records_and_pairs_are_named_and_nothing_is_written(small):
    kc, lib = small, pkg.lib()
    read_lens, alns, pairs = small_case()
    good = alns[7]  # read 4 of 100 bases on contig 0 (300 bases): cstart 100, cstop 200, rstart 0, rstop 100

    def forged(**kw):
        r = good.copy()
        for k, v in kw.items():
            r[k] = v
        return r

    bad = [forged(read=8), forged(read=0xFFFFFFFF), forged(ctg=3), forged(orient=2), forged(kind=3), forged(cstop=301), forged(cstart=200),
           forged(rstart=100), forged(rstop=101), forged(rstop=1025, rstart=1000)]
    for b in bad:
        with pytest.raises(M.BadRecord):
            M.ctg_links(LENS, read_lens, records([b]), None, **KW)
        device_links(kc, 3, read_lens, records([b]), None, expect=_lib.KC_ERR_INVALID_ARG, **KW)
        assert b"kc_ctg_links: record 0 " in lib.kc_last_error()
        many = np.concatenate([alns, records([b]), alns, records([b])])
        with pytest.raises(M.BadRecord) as e:
            M.ctg_links(LENS, read_lens, many, pairs, **KW)
        assert e.value.index == len(alns)
        device_links(kc, 3, read_lens, many, pairs, expect=_lib.KC_ERR_INVALID_ARG, **KW)
        assert b"record %d " % len(alns) in lib.kc_last_error()
    # pairs: an index out of range, a record of another read, a record of kind NONE
    for p, name, v in ((1, "aln0", len(alns)), (3, "aln1", 9), (0, "aln1", 4), (2, "aln0", 0xFFFFFFFE)):
        q = pairs.copy()
        q[p][name] = v
        with pytest.raises(M.BadPair) as e:
            M.ctg_links(LENS, read_lens, alns, q, **KW)
        assert e.value.index == p
        device_links(kc, 3, read_lens, alns, q, expect=_lib.KC_ERR_INVALID_ARG, **KW)
        assert b"kc_ctg_links: pair %d " % p in lib.kc_last_error()
        q[3]["aln0"] = 3  # a second bad pair behind it: the lowest is named
        device_links(kc, 3, read_lens, alns, q, expect=_lib.KC_ERR_INVALID_ARG, **KW)
        assert b"kc_ctg_links: pair %d " % p in lib.kc_last_error()
    # a bad record is named in front of a bad pair, a bad read in front of both
    q = pairs.copy()
    q[0]["aln0"] = 2
    device_links(kc, 3, read_lens, np.concatenate([alns, records([bad[2]])]), q, expect=_lib.KC_ERR_INVALID_ARG, **KW)
    assert b"record %d " % len(alns) in lib.kc_last_error()
    long_reads = read_lens[:5] + [1025, 100, 2000]
    with pytest.raises(M.BadRead) as e:
        M.ctg_links(LENS, long_reads, alns, pairs, **KW)
    assert e.value.index == 5
    device_links(kc, 3, long_reads, np.concatenate([alns, records([bad[2]])]), q, expect=_lib.KC_ERR_INVALID_ARG, **KW)
    assert b"kc_ctg_links: read 5 " in lib.kc_last_error()
    compare(kc, LENS, read_lens[:5] + [1024, 100, 1024], alns, pairs, **KW)
    # an odd number of reads, misaligned record arrays, a parameter out of range: with a context this time
    device_links(kc, 3, read_lens[:7], alns, None, expect=_lib.KC_ERR_INVALID_ARG, **KW)
    assert b"7 reads are no pairs" in lib.kc_last_error()
    device_links(kc, 3, read_lens, alns, pairs, n=4, shift=8, expect=_lib.KC_ERR_INVALID_ARG, **KW)
    assert b"16-byte aligned" in lib.kc_last_error()
    p = _lib.kc_link_params(**M.params(max_read_alns=65))
    cnt = C.c_uint64(5)
    assert lib.kc_ctg_links(kc._h, None, 0, None, 0, None, 1, C.byref(p), None, 0, None, C.byref(cnt), None) == _lib.KC_ERR_INVALID_ARG
    assert cnt.value == 5 and b"max_read_alns 65" in lib.kc_last_error()
    compare(kc, LENS, read_lens, alns, pairs, **KW)


def test_index_states_and_ranks():
    read_lens, alns, pairs = small_case()
    with pkg.KmerCounter(21) as kc:
        device_links(kc, 3, read_lens, alns, pairs, expect=_lib.KC_ERR_STATE, **KW)  # no index
        assert b"kc_ctg_links: no contig index" in pkg.lib().kc_last_error()
    with lengths_index(LENS) as kc:
        want = compare(kc, LENS, read_lens, alns, pairs, **KW)
        kc.clear_contig_index()
        device_links(kc, 3, read_lens, alns, pairs, expect=_lib.KC_ERR_STATE, **KW)
    with lengths_index(LENS) as kc:
        kc.reset()
        device_links(kc, 3, read_lens, alns, pairs, expect=_lib.KC_ERR_STATE, **KW)
    lens2 = [250, 400, 300, 7]  # a rebuilt index with the lengths of contigs 0 and 2 exchanged: the records fit no more
    with lengths_index(LENS) as kc:
        rng = np.random.default_rng(3)
        kc.index_contigs(*block_arrays([rand_seq(rng, n) for n in lens2]))
        device_links(kc, 4, read_lens, alns, pairs, expect=_lib.KC_ERR_INVALID_ARG, **KW)
        alns2 = alns.copy()
        alns2["ctg"] = np.where(alns["kind"] == M.KIND_NONE, 0, 2 - alns["ctg"])
        got = compare(kc, lens2, read_lens, alns2, pairs, **KW)
        assert got[2] == want[2]
    with lengths_index(LENS, rank_me=1, rank_n=2) as kc:
        compare(kc, LENS, read_lens, alns, pairs, **KW)


# ---- through the device's own steps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.LAYOUTS))
def test_after_the_devices_own_alignment_steps(name):
    """index_contigs -> align_reads -> align_gapped -> pair_inserts -> ctg_links over tests/links_cases.py's construction:
    the result is the model's, and it is what the construction says"""
    layout, gaps = LC.LAYOUTS[name]
    G = LC.genome(19)
    contigs = LC.contigs_of(G, layout)
    reads, places = LC.pairs_of(G, 19)
    b, o = read_arrays(reads)
    ctg_lens, read_lens = [len(c) for c in contigs], [len(r) for r in reads]
    kw = dict(insert_avg=LC.FRAGMENT, max_insert=1000, end_slack=0, max_overlap=50, max_splint_gap=50)
    with pkg.KmerCounter(LC.K) as kc:
        kc.index_contigs(*block_arrays(contigs))
        kc.submit_reads(b, np.full(len(b), ord("I"), dtype=np.uint8), o)
        res_before = [np.array(x) for x in kc.sorted_results()]
        looked = [np.array(x) for x in kc.lookup(res_before[0][:50])]
        kc.index_contigs(*block_arrays(contigs))
        alns, first, _ = kc.align_reads(b, o)
        gapped, _ = kc.align_gapped(b, o, alns)
        hist, pairs, ist = kc.pair_inserts(o, gapped, max_insert=1000)
        links, end_first, st, gap = kc.ctg_links(o, gapped, pairs, **kw)
        want = M.ctg_links(ctg_lens, read_lens, gapped, pairs, **kw)
        assert (links.tobytes(), end_first.tobytes(), st) == (want[0].tobytes(), want[1].tobytes(), want[2])
        same(device_links(kc, 3, read_lens, gapped, pairs, n=len(want[0]), **kw), want)
        LC.check_claims(links, st, gaps)
        assert [int(x) for x in links["from"]] == [1, 2, 3, 5] and [float(x) for x in gap] == [float(gaps[(1, 2)])] * 2 + [5.0, 5.0]
        assert st["span_cands"] == ist["cls"][D.PAIR_DIFF_CTG] > 0
        # the earlier calls answer as before
        alns2, first2, _ = kc.align_reads(b, o)
        assert alns2.tobytes() == alns.tobytes() and (first2 == first).all()
        assert kc.align_gapped(b, o, alns)[0].tobytes() == gapped.tobytes()
        assert kc.pair_inserts(o, gapped, max_insert=1000)[1].tobytes() == pairs.tobytes()
        assert all((x == np.array(y)).all() for x, y in zip(res_before, kc.sorted_results()))
        assert all((x == np.array(y)).all() for x, y in zip(looked, kc.lookup(res_before[0][:50])))
