"""tests/links_model.py against cases whose answer follows from the case alone (no GPU needed): a read laid across two or
three contigs by construction, pairs of a known fragment length across a known gap, and the mirror properties."""
import numpy as np
import pytest

import links_cases as LC
import links_model as M
from depth_model import NO_ALN, PAIR_DTYPE, rec, records

NONE_REC = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, M.KIND_NONE, (0, 0))


def piece(read, L, qs, qe, ctg, ctg_len, orient, side, e=0, score=None):
    """the record of the read's bases [qs, qe) (in the read's own direction) lying on contig ctg in orientation orient,
    e bases away from the contig's `side` end"""
    n = qe - qs
    cstart = e if side == "left" else ctg_len - e - n
    rstart = qs if orient == 0 else L - qe
    return rec(read, ctg, cstart, cstart + n, rstart=rstart, rstop=rstart + n, orient=orient, score=score)


def leaving(read, L, qs, qe, ctg, ctg_len, orient, e=0, **kw):
    """a piece that runs off its contig: through the right end iff it lies forward"""
    return piece(read, L, qs, qe, ctg, ctg_len, orient, "right" if orient == 0 else "left", e, **kw)


def entering(read, L, qs, qe, ctg, ctg_len, orient, e=0, **kw):
    return piece(read, L, qs, qe, ctg, ctg_len, orient, "left" if orient == 0 else "right", e, **kw)


def leave_end(ctg, orient):
    return 2 * ctg + (1 if orient == 0 else 0)


def enter_end(ctg, orient):
    return 2 * ctg + (0 if orient == 0 else 1)


def one_link(out):
    links, end_first, st = out
    assert len(links) == 2 and st["links"] == 1 and st["ends_linked"] == 2
    a, b = links
    assert (int(a["from"]), int(a["to"])) == (int(b["to"]), int(b["from"])) and int(a["from"]) < int(a["to"])
    assert a.tobytes()[8:] == b.tobytes()[8:]  # the same figures in both directions
    assert int(end_first[-1]) == 2 and all(int(end_first[e + 1]) - int(end_first[e]) == (1 if e in (a["from"], a["to"]) else 0)
                                           for e in range(len(end_first) - 1))
    return a


LENS = [300, 400, 250]


@pytest.mark.parametrize("gap", [0, 7, -20])
@pytest.mark.parametrize("oa,ob", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_one_read_across_two_contigs(gap, oa, ob):
    L = 100
    alns = records([leaving(0, L, 0, 50, 0, LENS[0], oa), entering(0, L, 50 + gap, L, 1, LENS[1], ob)])
    a = one_link(M.ctg_links(LENS, [L, 0], alns))
    assert {int(a["from"]), int(a["to"])} == {leave_end(0, oa), enter_end(1, ob)}
    assert (int(a["splints"]), int(a["spans"])) == (1, 0)
    assert int(a["splint_gap_min"]) == int(a["splint_gap_max"]) == int(a["splint_gap_sum"]) == gap
    assert (int(a["span_gap_min"]), int(a["span_gap_max"]), int(a["span_gap_sum"])) == (0, 0, 0)
    # the records the other way round; and the contigs the other way round: b leaves contig 1, a enters contig 0
    assert M.ctg_links(LENS, [L, 0], alns[::-1].copy())[0].tobytes() == M.ctg_links(LENS, [L, 0], alns)[0].tobytes()
    back = records([leaving(0, L, 0, 50, 1, LENS[1], ob), entering(0, L, 50 + gap, L, 0, LENS[0], oa)])
    b = one_link(M.ctg_links(LENS, [L, 0], back))
    assert {int(b["from"]), int(b["to"])} == {leave_end(1, ob), enter_end(0, oa)}


def test_end_slack_on_either_side_and_e_in_the_gap():
    L = 100
    for ea, eb, n in ((5, 0, 1), (6, 0, 0), (0, 5, 1), (0, 6, 0), (5, 5, 1), (6, 6, 0)):
        alns = records([leaving(0, L, 0, 50, 0, LENS[0], 0, e=ea), entering(0, L, 53, L, 1, LENS[1], 0, e=eb)])
        links, _, st = M.ctg_links(LENS, [L, 0], alns, end_slack=5)
        assert (len(links), st["splint_cands"], st["splints_gap_out"]) == (2 * n, n, 0), (ea, eb)
        if n:
            assert int(links[0]["splint_gap_sum"]) == 3 - ea - eb
    # slack 0: only alignments that stop at the very end
    alns = records([leaving(0, L, 0, 50, 0, LENS[0], 1, e=1), entering(0, L, 50, L, 1, LENS[1], 1)])
    assert len(M.ctg_links(LENS, [L, 0], alns, end_slack=0)[0]) == 0
    assert len(M.ctg_links(LENS, [L, 0], alns, end_slack=1)[0]) == 2


def test_gap_bounds():
    L = 200
    for gap, kept in ((30, True), (31, False), (-40, True), (-41, False)):
        alns = records([leaving(0, L, 0, 100, 0, LENS[0], 0), entering(0, L, 100 + gap, L, 1, LENS[1], 1)])
        links, _, st = M.ctg_links(LENS, [L, 0], alns, max_overlap=40, max_splint_gap=30)
        assert (len(links), st["splint_cands"], st["splints_gap_out"]) == ((2, 1, 0) if kept else (0, 0, 1)), gap
    # e moves a gap across the bound
    alns = records([leaving(0, L, 0, 100, 0, LENS[0], 0, e=2), entering(0, L, 100 - 39, L, 1, LENS[1], 0)])
    assert M.ctg_links(LENS, [L, 0], alns, max_overlap=40)[2]["splints_gap_out"] == 1


def test_a_read_over_three_contigs():
    L, mid = 300, 60  # the middle contig is 60 bases, all of it inside the read
    lens = [300, mid, 250]
    middle = rec(0, 1, 0, mid, rstart=100, rstop=160)  # forward: it enters through its left end and leaves through its right
    alns = records([leaving(0, L, 0, 100, 0, lens[0], 0), middle, entering(0, L, 160, L, 2, lens[2], 0)])
    links, _, st = M.ctg_links(lens, [L, 0], alns, max_splint_gap=59)
    assert [(int(x["from"]), int(x["to"])) for x in links] == [(1, 2), (2, 1), (3, 4), (4, 3)]  # a -> b, b -> c
    assert st["splints_gap_out"] == 1 and st["splint_cands"] == 2  # a -> c has gap 60
    links, _, st = M.ctg_links(lens, [L, 0], alns, max_splint_gap=60)
    assert [(int(x["from"]), int(x["to"])) for x in links] == [(1, 2), (1, 4), (2, 1), (3, 4), (4, 1), (4, 3)]
    assert [int(x["splint_gap_sum"]) for x in links] == [0, 60, 0, 0, 60, 0] and st["links"] == 3 and st["ends_linked"] == 4


def test_max_read_alns():
    L, n = 400, 4
    lens = [50] * n  # a chain of whole contigs inside one read, each entered and left
    alns = records([rec(0, u, 0, 50, rstart=60 * u, rstop=60 * u + 50) for u in range(n)])
    links, _, st = M.ctg_links(lens, [L, 0], alns, max_read_alns=n, max_splint_gap=10)
    assert st["reads_over_cap"] == 0 and st["splint_cands"] == n - 1 and st["splints_gap_out"] == (n - 1) * (n - 2) // 2
    assert [(int(x["from"]), int(x["to"])) for x in links if x["from"] < x["to"]] == [(2 * u + 1, 2 * u + 2) for u in range(n - 1)]
    links, _, st = M.ctg_links(lens, [L, 0], alns, max_read_alns=n - 1, max_splint_gap=10)
    assert len(links) == 0 and st["reads_over_cap"] == 1 and st["splint_cands"] == 0 and st["passed"] == n
    # a record that does not pass does not count towards the cap
    alns2 = records(list(alns[:n - 1]) + [rec(0, n - 1, 0, 50, rstart=60 * (n - 1), rstop=60 * (n - 1) + 50, score=1)])
    links, _, st = M.ctg_links(lens, [L, 0], alns2, max_read_alns=n - 1, max_splint_gap=10, min_score=2)
    assert st["reads_over_cap"] == 0 and st["filtered"] == 1 and st["splint_cands"] == n - 2


def test_equal_starts_or_stops_and_one_contig_give_nothing():
    L = 100
    same_qs = records([leaving(0, L, 10, 50, 0, LENS[0], 0), entering(0, L, 10, 60, 1, LENS[1], 0)])
    same_qe = records([leaving(0, L, 10, 60, 0, LENS[0], 0), entering(0, L, 20, 60, 1, LENS[1], 0)])
    for alns in (same_qs, same_qe):
        links, _, st = M.ctg_links(LENS, [L, 0], alns)
        assert len(links) == 0 and st["splint_cands"] == st["splints_gap_out"] == 0 and st["passed"] == 2
    # two records on one contig: a circle is not this call's; NONE records and filtered ones are counted and ignored
    alns = records([leaving(0, L, 0, 50, 0, LENS[0], 0), entering(0, L, 50, L, 0, LENS[0], 0), NONE_REC])
    links, _, st = M.ctg_links(LENS, [L, 0], alns)
    assert len(links) == 0 and (st["records"], st["none"], st["passed"]) == (3, 1, 2)
    links, _, st = M.ctg_links(LENS, [L, 0], records([leaving(0, L, 0, 50, 0, LENS[0], 0), entering(0, L, 50, L, 1, LENS[1], 0)]), min_len=51)
    assert len(links) == 0 and st["filtered"] == 2


def span_case(o0, o1, gap, f, lens=(1000, 800), L=100):
    """a fragment of f bases over contig 0, a gap and contig 1, each contig lying as o0 / o1 say: mate 0 starts the
    fragment on contig 0, mate 1 ends it on contig 1.  Returns (alns, pairs)."""
    d0 = 300  # from mate 0's first base to the end of contig 0 it points at
    d1 = f - gap - d0
    assert L <= d1 <= lens[1]
    # mate 0 points at contig 0's right end iff it lies forward on it
    m0 = rec(0, 0, lens[0] - d0, lens[0] - d0 + L, orient=0) if o0 == 0 else rec(0, 0, d0 - L, d0, orient=1)
    m1 = rec(1, 1, d1 - L, d1, orient=1) if o1 == 0 else rec(1, 1, lens[1] - d1, lens[1] - d1 + L, orient=0)
    pairs = np.zeros(1, dtype=PAIR_DTYPE)
    pairs[0] = (0, 1, 0, 2, (0, 0, 0))
    return records([m0, m1]), pairs


@pytest.mark.parametrize("o0,o1", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("gap", [0, 25, -30])
def test_spans(o0, o1, gap):
    lens, f = [1000, 800], 700
    alns, pairs = span_case(o0, o1, gap, f)
    a = one_link(M.ctg_links(lens, [100, 100], alns, pairs, insert_avg=f, max_insert=900))
    assert {int(a["from"]), int(a["to"])} == {1 if o0 == 0 else 0, 2 if o1 == 0 else 3}
    assert (int(a["splints"]), int(a["spans"])) == (0, 1) and int(a["span_gap_min"]) == int(a["span_gap_max"]) == int(a["span_gap_sum"]) == gap
    assert (int(a["splint_gap_min"]), int(a["splint_gap_max"]), int(a["splint_gap_sum"])) == (0, 0, 0)
    # d0 + d1 = f - gap: at max_insert and one over
    links, _, st = M.ctg_links(lens, [100, 100], alns, pairs, insert_avg=f - gap, max_insert=f - gap)
    assert len(links) == 2 and st["span_cands"] == 1 and int(links[0]["span_gap_sum"]) == 0
    if f - gap - 1 >= 1:
        links, _, st = M.ctg_links(lens, [100, 100], alns, pairs, insert_avg=f - gap - 1, max_insert=f - gap - 1)
        assert len(links) == 0 and st["span_cands"] == 0 and st["spans_too_far"] == 1
    # without pairs, with a mate missing, and with both mates on one contig there is no span
    assert len(M.ctg_links(lens, [100, 100], alns, None, insert_avg=f)[0]) == 0
    for x in ((NO_ALN, 1), (0, NO_ALN), (NO_ALN, NO_ALN)):
        q = pairs.copy()
        q[0]["aln0"], q[0]["aln1"] = x
        assert M.ctg_links(lens, [100, 100], alns, q, insert_avg=f)[2]["span_cands"] == 0
    same = alns.copy()
    same["ctg"] = 0
    same["cstart"], same["cstop"] = 100, 200
    st = M.ctg_links(lens, [100, 100], same, pairs, insert_avg=f)[2]
    assert st["span_cands"] == st["spans_too_far"] == 0


def test_a_mate_hanging_over_its_contig_end_is_projected():
    # mate 0 forward, its first 10 bases in front of contig 0 (soft-clipped): d0 = len - (0 - 10)
    lens = [200, 800]
    alns = records([rec(0, 0, 0, 90, rstart=10, rstop=100), rec(1, 1, 100, 190, rstart=0, rstop=90, orient=1)])
    pairs = np.zeros(1, dtype=PAIR_DTYPE)
    pairs[0] = (0, 1, 0, 2, (0, 0, 0))
    links, _, st = M.ctg_links(lens, [100, 100], alns, pairs, insert_avg=500, max_insert=500)
    assert int(links[0]["span_gap_sum"]) == 500 - 210 - (190 + 10)


def test_a_splint_and_a_span_on_one_link():
    lens, L = [1000, 800], 100
    alns, pairs = span_case(0, 0, 12, 700)
    splint = [leaving(2, L, 0, 40, 0, lens[0], 0), entering(2, L, 52, L, 1, lens[1], 0)]
    alns = records(list(alns) + splint + splint)
    pairs = np.concatenate([pairs, np.array([(NO_ALN, NO_ALN, 0, 0, (0, 0, 0))], dtype=PAIR_DTYPE)])
    a = one_link(M.ctg_links(lens, [L] * 4, alns, pairs, insert_avg=700))
    # the doubled records of read 2: a x b over all ordered pairs gives 2 x 2 splints
    assert (int(a["from"]), int(a["to"]), int(a["splints"]), int(a["spans"])) == (1, 2, 4, 1)
    assert (int(a["splint_gap_sum"]), int(a["span_gap_sum"]), int(a["splint_gap_min"]), int(a["span_gap_max"])) == (48, 12, 12, 12)
    st = M.ctg_links(lens, [L] * 4, alns, pairs, insert_avg=700)[2]
    assert (st["links"], st["links_both"], st["links_splint_only"], st["links_span_only"]) == (1, 1, 0, 0)
    st = M.ctg_links(lens, [L] * 4, alns, None, insert_avg=700)[2]
    assert (st["links"], st["links_both"], st["links_splint_only"], st["links_span_only"]) == (1, 0, 1, 0)


def random_case(rng, n_ctgs=6, nreads=40):
    lens = [int(x) for x in rng.integers(60, 400, size=n_ctgs)]
    read_lens = [int(x) for x in rng.integers(80, 200, size=nreads)]
    rows = []
    for r, L in enumerate(read_lens):
        cut = int(rng.integers(20, L - 20))
        u, v = (int(x) for x in rng.choice(n_ctgs, size=2, replace=False))
        oa, ob = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        g = int(rng.integers(-10, 20))  # between the two pieces, in the read
        n_a, n_b = min(cut, lens[u] - 6), min(L - cut - g, lens[v] - 6)
        rows.append(leaving(r, L, cut - n_a, cut, u, lens[u], oa, e=int(rng.integers(0, 7))))
        rows.append(entering(r, L, cut + g, cut + g + n_b, v, lens[v], ob, e=int(rng.integers(0, 7))))
    alns = records(rows)
    best = {}
    for i, a in enumerate(alns):
        best.setdefault(int(a["read"]), i)
    pairs = np.zeros(nreads // 2, dtype=PAIR_DTYPE)
    for q in range(nreads // 2):
        pairs[q] = (best.get(2 * q, NO_ALN), best.get(2 * q + 1, NO_ALN), 0, 0, (0, 0, 0))
    return lens, read_lens, alns, pairs


def revcomp_reads(alns, which):
    """the same alignments of the reads' reverse complements: the read in contig orientation is the same text"""
    out = alns.copy()
    flip = np.isin(out["read"], which)
    out["orient"][flip] ^= 1
    return out


def flip_contig(alns, u, len_u, read_lens):
    """the same alignments against contig u's reverse complement"""
    out = alns.copy()
    for a in out:
        if int(a["ctg"]) == u and int(a["kind"]) != M.KIND_NONE:
            L = read_lens[int(a["read"])]
            a["cstart"], a["cstop"] = len_u - int(a["cstop"]), len_u - int(a["cstart"])
            a["rstart"], a["rstop"] = L - int(a["rstop"]), L - int(a["rstart"])
            a["orient"] ^= 1
    return out


def as_set(links, swap=None):
    def end(e):
        return e ^ 1 if swap is not None and e >> 1 == swap else e
    return sorted((end(int(x["from"])), end(int(x["to"]))) + tuple(int(x[n]) for n in M.LINK_DTYPE.names[2:]) for x in links)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mirrors_and_shuffles(seed):
    rng = np.random.default_rng(seed)
    lens, read_lens, alns, pairs = random_case(rng)
    kw = dict(end_slack=5, max_overlap=15, max_splint_gap=12, insert_avg=300, max_insert=500)
    want = M.ctg_links(lens, read_lens, alns, None, **kw)
    assert want[2]["splint_cands"] > 5 and want[2]["splints_gap_out"] > 0 and want[2]["passed"] > want[2]["splint_cands"]
    # shuffled records: one byte string (without pairs, which hold indices)
    perm = rng.permutation(len(alns))
    got = M.ctg_links(lens, read_lens, alns[perm], None, **kw)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    inv = np.argsort(perm)
    q = pairs.copy()
    for n in ("aln0", "aln1"):
        q[n] = [NO_ALN if int(i) == NO_ALN else inv[int(i)] for i in pairs[n]]
    with_pairs = M.ctg_links(lens, read_lens, alns, pairs, **kw)
    got = M.ctg_links(lens, read_lens, alns[perm], q, **kw)
    assert got[0].tobytes() == with_pairs[0].tobytes() and got[2] == with_pairs[2]
    # the reverse complement of a read is the same splints
    got = M.ctg_links(lens, read_lens, revcomp_reads(alns, list(range(0, len(read_lens), 3))), None, **kw)
    assert got[0].tobytes() == want[0].tobytes() and got[2] == want[2]
    # the reverse complement of a contig is the same links with its two ends' numbers swapped, spans included
    for u in (0, 3):
        got = M.ctg_links(lens, read_lens, flip_contig(alns, u, lens[u], read_lens), pairs, **kw)
        assert as_set(got[0], swap=u) == as_set(with_pairs[0]) and got[2] == with_pairs[2]


def test_arguments_and_validity():
    alns = records([rec(0, 0, 250, 300, rstop=50), rec(0, 1, 0, 50, rstart=50, rstop=100)])
    for kw in (dict(end_slack=1025), dict(max_overlap=65536), dict(max_splint_gap=1025), dict(insert_avg=0), dict(insert_avg=1001),
               dict(max_insert=65536, insert_avg=5), dict(max_read_alns=1), dict(max_read_alns=65), dict(flags=1)):
        with pytest.raises(M.BadArg):
            M.ctg_links(LENS, [100, 0], alns, **kw)
    for kw in (dict(end_slack=1024), dict(max_overlap=65535), dict(max_splint_gap=1024), dict(insert_avg=1, max_insert=1),
               dict(insert_avg=65535, max_insert=65535), dict(max_read_alns=2), dict(max_read_alns=64)):
        assert len(M.ctg_links(LENS, [100, 0], alns, **kw)[0]) == 2
    with pytest.raises(M.BadArg):
        M.ctg_links(LENS, [100, 0, 0], alns)
    with pytest.raises(M.BadRead) as e:
        M.ctg_links(LENS, [100, 1025], alns)
    assert e.value.index == 1
    with pytest.raises(M.BadRecord) as e:
        M.ctg_links(LENS, [100, 0], records([alns[0], rec(0, 1, 0, 50, rstart=51, rstop=101)]))
    assert e.value.index == 1
    pairs = np.zeros(1, dtype=PAIR_DTYPE)
    pairs[0] = (0, 1, 0, 0, (0, 0, 0))  # record 1 is read 0's, not read 1's
    with pytest.raises(M.BadPair) as e:
        M.ctg_links(LENS, [100, 0], alns, pairs)
    assert e.value.index == 0
    # no records: no links, an all-zero end_first
    links, end_first, st = M.ctg_links(LENS, [100, 0], records([]))
    assert len(links) == 0 and len(end_first) == 7 and not end_first.any() and st["reads"] == 2 and st["records"] == 0


@pytest.mark.parametrize("name", sorted(LC.LAYOUTS))
def test_the_end_to_end_construction_holds_for_the_rules_alone(name):
    """the construction tests/test_gpu_ctg_links.py runs through the device's alignment steps, here with the records
    laid out by geometry: right(0) -- left(1) at +10 (or -20 where the contigs overlap), right(1) -- right(2) at +5
    into the reversed contig, and nothing else"""
    import depth_model as D
    layout, gaps = LC.LAYOUTS[name]
    G = LC.genome(19)
    reads, places = LC.pairs_of(G, 19)
    alns = LC.geometric_records(layout, places)
    ctg_lens, read_lens = [b - a for a, b, _ in layout], [len(r) for r in reads]
    _, pairs, ist = D.pair_inserts(ctg_lens, read_lens, alns, 1000)
    assert ist["cls"][D.PAIR_DIFF_CTG] > 0
    links, end_first, st = M.ctg_links(ctg_lens, read_lens, alns, pairs, insert_avg=LC.FRAGMENT, max_insert=1000, end_slack=0, max_overlap=50,
                                       max_splint_gap=50)
    LC.check_claims(links, st, gaps)
    assert st["span_cands"] == ist["cls"][D.PAIR_DIFF_CTG]
    assert [int(x) for x in end_first] == [0, 0, 1, 2, 3, 3, 4] and (links["from"] == [1, 2, 3, 5]).all() and (links["to"] == [2, 1, 5, 3]).all()
