"""The host model of kc_build_unitigs (tests/unitig_model.py) against hand cases whose unitigs are written out here, and
against the properties DESIGN section 14 states, on random result sets.  No GPU, no library: the model is the yardstick
the device tests compare with, so it is checked on its own first."""
import numpy as np
import pytest

import unitig_model as M


def results_from(seqs, k, count=2, first_wins=False):
    """The result set a counter would keep for these sequences when every k-mer with both neighbours survives: the k-mer
    at position i of a sequence, for 1 <= i <= len - k - 1, canonical, with the neighbouring bases as its extensions
    (complemented and swapped where the canonical form is the reverse complement).  Two occurrences that disagree on an
    extension are an error unless first_wins (random sets: the first occurrence's extensions stay)."""
    R = {}
    for s in seqs:
        for i in range(1, len(s) - k):
            t, l, r = s[i:i + k], s[i - 1], s[i + k]
            x = M.canonical(t)
            if x != t:
                l, r = M.comp(r), M.comp(l)
            if x in R:
                assert first_wins or R[x][1:] == (l, r), (x, R[x], l, r)
                R[x] = (R[x][0] + count, R[x][1], R[x][2])
            else:
                R[x] = (count, l, r)
    return R


def texts(R, k):
    return [u[0] for u in M.unitigs(R, k)[0]]


# ---- hand cases: the expected strings are written out ------------------------------------------------------------------
def test_linear_path():
    # the five 5-mers with both neighbours in GATTACAGGCT: ATTAC TTACA TACAG ACAGG CAGGC, one path.  Its head ATTAC is
    # smaller than the twin path's head CAGGC (the canonical form of the tail), so the path is written as it reads.
    R = results_from(["GATTACAGGCT"], 5, count=3)
    assert sorted(R) == ["ACAGG", "ATTAC", "CAGGC", "CTGTA", "TGTAA"]
    units, st = M.unitigs(R, 5)
    assert units == [("ATTACAGGC", 15, 3, 5)]
    assert st == dict(kmers=5, unitigs=1, singletons=0, circular=0, bases=9, longest=9)


def test_path_ended_by_a_purged_neighbour():
    # TACAG (canonical CTGTA) was purged, as a fork's k-mer is: the path falls in two, ordered by their heads ACAGG < ATTAC
    R = results_from(["GATTACAGGCT"], 5)
    del R["CTGTA"]
    assert texts(R, 5) == ["ACAGGC", "ATTACA"]


def test_one_sided_disagreement_ends_the_path():
    # TACAG's left extension names G where TTACA stands with T in front (another, stronger predecessor won the vote): TTACA's
    # right extension still leads to TACAG, but the two sides do not agree, so there is no link -- in either direction.
    # TACAG ACAGG CAGGC remain a path; its twin's head CAGGC is smaller than its own head's canonical CTGTA, so the
    # reverse complement GCCTGTA is what is written.
    R = results_from(["GATTACAGGCT"], 5)
    c, l, r = R["CTGTA"]  # = revcomp(TACAG): its right extension is the complement of TACAG's left
    assert (l, r) == ("C", "A")
    R["CTGTA"] = (c, l, "C")
    assert M.successor(R, ("TGTAA", -1)) is None and M.successor(R, ("CTGTA", 1)) is None
    assert texts(R, 5) == ["ATTACA", "GCCTGTA"]


def test_hairpin_ends_the_walk():
    # AACGT followed by T is ACGTT, AACGT's own reverse complement (around the palindromic 4-mer ACGT): no self-link.
    # GCAAC CAACG AACGT is a path; the twin's head AACGT is the smaller, so the reverse complement of GCAACGT is written.
    R = results_from(["GGCAACGTT"], 5)
    assert sorted(R) == ["AACGT", "CAACG", "GCAAC"]
    assert M.successor(R, ("AACGT", 1)) is None and M.successor(R, ("AACGT", -1)) == ("CAACG", -1)
    units, st = M.unitigs(R, 5)
    assert units == [("ACGTTGC", 6, 2, 3)]
    assert st["singletons"] == 0 and st["circular"] == 0


def test_cycle_is_cut_at_its_smallest_kmer():
    # the circle AACCGTCT (8 bases, 8 distinct 5-mers), read twice round and six bases on; the smallest canonical
    # 5-mer of the circle is AACCG, on the strand written here, so the cycle opens in front of it: 5 + 8 - 1 bases
    circle = "AACCGTCT"
    R = results_from([circle * 2 + circle[:6]], 5, count=2, first_wins=True)
    assert len(R) == 8 and min(R) == "AACCG"
    units, st = M.unitigs(R, 5)
    assert [u[0] for u in units] == ["AACCGTCTAACC"]
    assert units[0][3] == 8 and st["circular"] == 1 and st["unitigs"] == 1
    # the same circle given as its reverse complement, starting elsewhere: the same result set, the same unitig
    rc = M.revcomp(circle)
    rc = rc[3:] + rc[:3]
    R2 = results_from([rc * 2 + rc[:6]], 5, count=2, first_wins=True)
    assert sorted(R2) == sorted(R)
    assert texts(R2, 5) == ["AACCGTCTAACC"]


def test_cycle_of_two_kmers():
    # the circle of two bases AC at k = 5: ACACA and CACAC (canonical CACAC vs GTGTG) follow each other
    R = {"ACACA": (4, "C", "C"), "CACAC": (4, "A", "A")}
    assert M.successor(R, ("ACACA", 1)) == ("CACAC", 1) and M.successor(R, ("CACAC", 1)) == ("ACACA", 1)
    units, st = M.unitigs(R, 5)
    assert units == [("ACACAC", 8, 4, 2)] and st["circular"] == 1


def test_palindromic_kmer_at_even_k_is_a_unitig_of_its_own():
    # ACGCGT is its own reverse complement; TACGCG in front of it and CGCGTG behind it both lead to it, and neither links
    R = results_from(["TTACGCGTGA"], 6)
    assert sorted(R) == ["ACGCGT", "CACGCG", "CGCGTA"]
    units, st = M.unitigs(R, 6)
    assert [u[0] for u in units] == ["ACGCGT", "CACGCG", "CGCGTA"]
    assert st["singletons"] == 3 and st["unitigs"] == 3 and st["longest"] == 6


def test_isolated_kmers():
    # extensions that lead nowhere: every k-mer alone, written in its canonical form, in key order
    R = {"TGCAA": (7, "A", "C"), "AAGGC": (65535, "T", "T"), "CCCTA": (2, "G", "G")}
    units, st = M.unitigs(R, 5)
    assert units == [("AAGGC", 65535, 65535, 1), ("CCCTA", 2, 2, 1), ("TGCAA", 7, 7, 1)]
    assert st == dict(kmers=3, unitigs=3, singletons=3, circular=0, bases=15, longest=5)


def test_homopolymer_does_not_link_to_itself():
    R = {"AAAAA": (9, "A", "A")}
    assert M.successor(R, ("AAAAA", 1)) is None and M.successor(R, ("AAAAA", -1)) is None
    assert texts(R, 5) == ["AAAAA"]


def test_depth_is_the_mean_rounded_half_up_and_clipped():
    R = results_from(["GATTACAGGCT"], 5)
    R = {x: (c, l, r) for (x, (_, l, r)), c in zip(sorted(R.items()), (2, 3, 3, 2, 2))}  # 12 / 5 = 2.4
    assert M.unitigs(R, 5)[0][0][1:3] == (12, 2)
    R = {x: (c, l, r) for (x, (_, l, r)), c in zip(sorted(R.items()), (2, 3, 3, 2, 3))}  # 13 / 5 = 2.6
    assert M.unitigs(R, 5)[0][0][1:3] == (13, 3)
    R = {"ACACA": (3, "C", "C"), "CACAC": (2, "A", "A")}  # 5 / 2 = 2.5: half goes up
    assert M.unitigs(R, 5)[0][0][1:3] == (5, 3)
    R = {"ACACA": (65535, "C", "C"), "CACAC": (65535, "A", "A")}
    assert M.unitigs(R, 5)[0][0][1:3] == (131070, 65535)


def test_block_layout():
    units = [("ACGTA", 10, 10, 1), ("CCCTAGG", 7, 2, 3)]
    seqs, depths, offsets, sums = M.block(units)
    assert seqs == b"ACGTA_CCCTAGG_"
    assert depths.tolist() == [10] * 5 + [0] + [2] * 7 + [0] and depths.dtype == np.uint16
    assert offsets.tolist() == [0, 6, 14] and sums.tolist() == [10, 7]


# ---- properties on random result sets ------------------------------------------------------------------------------------
def random_results(rng, k):
    """k-mers of a random genome with repeats, a circle and mutated copies; some purged, some extensions changed: forks,
    one-sided disagreements, dead ends, cycles.  At even k palindromic k-mers are put in on purpose."""
    g = "".join(rng.choice(list("ACGT"), size=1500))
    seqs = [g, g[200:500] + g[900:1100]]  # a repeat joined differently
    m = list(g[300:800])
    for j in rng.integers(0, len(m), size=6):
        m[j] = "ACGT"[int(rng.integers(0, 4))]
    seqs.append("".join(m))
    circle = "".join(rng.choice(list("ACGT"), size=k + 40))
    seqs.append(circle * 2 + circle[:k + 1])
    seqs.append("AC" * (k + 2))  # a cycle of two k-mers
    if k % 2 == 0:
        h = "".join(rng.choice(list("ACGT"), size=k // 2))
        seqs.append("GATTC" + h + M.revcomp(h) + "CTTGA")
    seqs.append(M.revcomp(g[1000:1300]))
    R = results_from(seqs, k, first_wins=True)
    keys = sorted(R)
    for x in rng.choice(keys, size=len(keys) // 40, replace=False):
        del R[x]
    keys = sorted(R)
    for x in rng.choice(keys, size=len(keys) // 40, replace=False):
        c, l, r = R[x]
        if rng.random() < 0.5:
            l = "ACGT"[int(rng.integers(0, 4))]
        else:
            r = "ACGT"[int(rng.integers(0, 4))]
        R[x] = (int(rng.integers(2, 70000)) % 65536 or 2, l, r)
    return R


def nodes_of(text, k):
    out = []
    for i in range(len(text) - k + 1):
        t = text[i:i + k]
        x = M.canonical(t)
        out.append((x, 1 if t == x else -1))
    return out


@pytest.mark.parametrize("k", [21, 22, 33])
def test_properties_on_random_result_sets(k):
    rng = np.random.default_rng(7000 + k)
    R = random_results(rng, k)
    assert len(R) > 1500
    # links: at most one predecessor, and v -> w iff twin(w) -> twin(v)
    succ, preds, nlinks = {}, {}, 0
    for x in R:
        for s in (1, -1):
            w = M.successor(R, (x, s))
            succ[(x, s)] = w
            if w is not None:
                nlinks += 1
                assert w not in preds, "two predecessors"
                preds[w] = (x, s)
    assert nlinks > len(R)
    for v, w in succ.items():
        if w is not None:
            assert succ[M.twin(w)] == M.twin(v)
            assert M.predecessor(R, w) == v
    units, st = M.unitigs(R, k)
    seen, heads, cycles, lone = set(), [], 0, 0
    for text, ksum, depth, m in units:
        nodes = nodes_of(text, k)
        assert len(nodes) == m == len(text) - k + 1
        for v in nodes:  # every k-mer on exactly one unitig
            assert v[0] in R and v[0] not in seen
            seen.add(v[0])
        for a, b in zip(nodes, nodes[1:]):  # consecutive k-mers are linked
            assert succ[a] == b
        # no unitig can be extended: nothing follows its tail and nothing leads to its head, or it is a cycle cut in front of
        # its smallest k-mer on the + strand
        nx, pv = succ[nodes[-1]], preds.get(nodes[0])
        if nx is None:
            assert pv is None
        else:
            assert nx == nodes[0] and pv == nodes[-1]
            assert nodes[0] == (min(v[0] for v in nodes), 1)
            cycles += 1
        # of the path and its twin, the one with the smaller head; a lone k-mer as (x,+)
        if m == 1:
            assert nodes[0][1] == 1
            lone += 1
        else:
            assert nodes[0][0] < nodes[-1][0]
        assert ksum == sum(R[v[0]][0] for v in nodes)
        assert depth == min(65535, (2 * ksum + m) // (2 * m))
        heads.append(nodes[0][0])
    assert seen == set(R)
    assert heads == sorted(heads) and len(set(heads)) == len(heads)  # ascending by head key
    assert cycles >= 1 and lone >= 1
    if k % 2 == 0:
        pal = [x for x in R if x == M.revcomp(x)]
        assert pal and all((x, R[x][0], min(65535, R[x][0]), 1) in units for x in pal)
    assert st == dict(kmers=len(R), unitigs=len(units), singletons=lone, circular=cycles, bases=sum(len(u[0]) for u in units),
                      longest=max(len(u[0]) for u in units))


def test_results_dict_reads_packed_keys():
    k = 33
    s = "ACGTTGCAAGGCTTAACCGGTTAACGTACGATCG"[:k]
    words = np.zeros((1, 2), dtype=np.uint64)
    for i, c in enumerate(s):
        words[0, i // 32] |= np.uint64("ACGT".index(c) << (2 * (31 - i % 32)))
    R = M.results_dict(words, np.array([5], dtype=np.uint16), np.array([ord("A")], dtype=np.uint8), np.array([ord("T")], dtype=np.uint8), k)
    assert R == {s: (5, "A", "T")}
