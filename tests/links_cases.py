"""A genome cut into contigs with known gaps between them, and error-free pairs of one fragment length over it: the
construction behind the by-construction claims of tests/test_links_model.py (records by geometry, no device) and of
tests/test_gpu_ctg_links.py (records by the device's own alignment steps)."""
import numpy as np

from depth_model import rec, records

K = 21
READ_LEN = 150
FRAGMENT = 400  # every pair's fragment length: the insert_avg of the calls
# (genome start, genome stop, reversed) of every contig; the ends that are neighbours in the genome and the gap between them
LAYOUTS = {
    "gaps": ([(0, 1000, 0), (1010, 2000, 0), (2005, 3000, 1)], {(1, 2): 10, (3, 5): 5}),
    "overlap": ([(0, 1000, 0), (980, 2000, 0), (2005, 3000, 1)], {(1, 2): -20, (3, 5): 5}),
}
RC = str.maketrans("ACGT", "TGCA")


def revc(s):
    return s.translate(RC)[::-1]


def genome(seed, n=3000):
    rng = np.random.default_rng(seed)
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def contigs_of(G, layout):
    return [revc(G[a:b]) if r else G[a:b] for a, b, r in layout]


def pairs_of(G, seed, depth=8):
    """(reads, placements): reads 2p and 2p + 1 are the two ends of a FRAGMENT-base piece of G, in either order;
    placements[i] = (genome start, genome stop, reversed) of read i"""
    rng = np.random.default_rng(seed)
    n = len(G) * depth // (2 * READ_LEN)
    reads, places = [], []
    for a in sorted(int(x) for x in rng.integers(0, len(G) - FRAGMENT + 1, size=n)):
        f = G[a:a + FRAGMENT]
        pair = [(f[:READ_LEN], (a, a + READ_LEN, 0)), (revc(f[-READ_LEN:]), (a + FRAGMENT - READ_LEN, a + FRAGMENT, 1))]
        if int(rng.integers(0, 2)):
            pair.reverse()
        for text, where in pair:
            reads.append(text)
            places.append(where)
    return reads, places


def geometric_records(layout, places):
    """the exact alignment of every read to every contig it shares at least K bases with, clipped at the contig's ends,
    as kc_align_gapped writes it: contig coordinates, and the read's in contig orientation"""
    rows = []
    for i, (s, e, rr) in enumerate(places):
        for u, (cs, ce, cr) in enumerate(layout):
            os_, oe = max(s, cs), min(e, ce)
            if oe - os_ < K:
                continue
            if cr == 0:
                rows.append(rec(i, u, os_ - cs, oe - cs, rstart=os_ - s, rstop=oe - s, orient=rr))
            else:
                rows.append(rec(i, u, ce - oe, ce - os_, rstart=e - oe, rstop=e - os_, orient=rr ^ 1))
    return records(rows)


def check_claims(links, stats, gaps):
    """what follows from the construction alone: the links are exactly the genome's neighbours, every gap is the true one"""
    got = {(int(x["from"]), int(x["to"])): x for x in links if x["from"] < x["to"]}
    assert set(got) == set(gaps), sorted(got)
    for ends, gap in gaps.items():
        x = got[ends]
        assert int(x["splints"]) > 0 and int(x["spans"]) > 0, x
        assert int(x["splint_gap_min"]) == int(x["splint_gap_max"]) == gap, x
        assert int(x["span_gap_min"]) == int(x["span_gap_max"]) == gap, x
        assert int(x["splint_gap_sum"]) == gap * int(x["splints"]) and int(x["span_gap_sum"]) == gap * int(x["spans"])
    assert stats["links"] == stats["links_both"] == len(gaps) and stats["ends_linked"] == 2 * len(gaps)
    assert stats["splints_gap_out"] == 0 and stats["spans_too_far"] == 0 and stats["reads_over_cap"] == 0
