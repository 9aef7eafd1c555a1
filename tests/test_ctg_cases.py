"""tests/ctg_cases.py against the C oracle's statement-for-statement restatement of the contig pass: what every case
expects by construction is what the oracle keeps, in every order of the contigs, and every family holds the cases it is
for.  No GPU."""
import numpy as np
import pytest

import ctg_cases as G
from oracle import cpu_oracle as O

KS = [21, 30, 31, 32, 33, 63, 64, 95, 125]


def oracle_results(k, dmin_thres, reads, ctgs, depths):
    o = O.Oracle(k, dmin_thres=dmin_thres, nranks=3, nthreads=1)
    o.add_reads(*reads)
    for c, d in zip(ctgs, depths):
        o.add_ctg(c, d)
    res = o.finalize()
    st = o.stats()
    o.close()
    assert st["dropped"] == 0
    return res, st


def check_against_the_oracle(cases, k, dmin_thres, seed=21):
    reads = G.emit_reads(cases, k, seed)
    assert len(reads[2]) - 1 == sum(c.reads.occurrences for c in cases)
    want = G.expected_results(cases, dmin_thres)
    est = G.expected_stats(cases, dmin_thres)
    by_key = {c.key: c for c in cases}
    assert len(by_key) == len(cases)
    for order in (None, 1, 2):
        ctgs, depths = G.emit_ctgs(cases, seed=order)
        got, st = oracle_results(k, dmin_thres, reads, ctgs, depths)
        assert got[0].shape[1] == G.num_words(k)
        kept = {tuple(int(x) for x in got[0][i]): (int(got[1][i]), chr(got[2][i]), chr(got[3][i])) for i in range(len(got[1]))}
        bad = [(c.name, kept.get(c.key), c.result(dmin_thres)) for c in cases if kept.get(c.key) != c.result(dmin_thres)]
        assert not bad, (order, bad[:8])
        for g, w, name in zip(got, want, ("keys", "counts", "left", "right")):
            assert g.shape == w.shape and (g == w).all(), (order, name)
        assert (st["total_kmers"], st["sum_counts"]) == (est["total_kmers"], est["sum_counts"])
    for c in cases[::13]:  # the packing is the oracle's
        assert (O.pack_kmer(c.canon) == np.array(c.key, dtype=np.uint64)).all()


@pytest.mark.parametrize("dmin_thres", G.DMIN_THRES)
@pytest.mark.parametrize("k", KS)
def test_families_match_the_oracle(k, dmin_thres):
    check_against_the_oracle(G.families(k), k, dmin_thres)


def test_seam_cases_match_the_oracle():
    check_against_the_oracle(G.seam_cases(21, 600), 21, 2)


@pytest.mark.parametrize("dmin_thres", G.DMIN_THRES)
@pytest.mark.parametrize("k", [21, 32])
def test_families_hold_what_they_are_for(k, dmin_thres):
    cases = G.families(k)
    fam = lambda f: [c for c in cases if c.family == f]
    floor = max(2, dmin_thres)
    # read side x one good occurrence: the reads' line where they keep K, the contig's everywhere else
    rs = fam("read-side")
    assert sorted({c.tags["kind"] for c in rs}) == sorted(G.READ_SIDES) and {o[3] for c in rs for o in c.occs} == {"+", "-"}
    for c in rs:
        kept = c.reads.result(dmin_thres)
        assert (kept is not None) == (c.tags["kind"] == "kept"), c.name
        assert c.reads.occurrences == {"absent": 0, "singleton": 1, "kept": 6, "fork-left": 12, "no-vote-right": 6, "both-missing": 6}[c.tags["kind"]]
        assert c.result(dmin_thres) == (kept if kept else c.ctg_result(dmin_thres)) and c.ctg_result(dmin_thres)[0] == 7
        assert c.ctg_result(dmin_thres)[1:] != (kept or (0, "", ""))[1:]  # the two lines can be told apart
    votes = {c.tags["kind"]: c.reads.exts(dmin_thres) for c in rs}
    # (in the canonical frame: which side forks or has no vote depends on the strand K is)
    assert sorted(votes["fork-left"], key="FACGT".index)[0] == "F" and votes["fork-left"].count("F") == 1 and "X" not in votes["fork-left"]
    assert sorted(votes["no-vote-right"], key="XACGT".index)[0] == "X" and votes["no-vote-right"].count("X") == 1 and "F" not in votes["no-vote-right"]
    assert votes["both-missing"] == ("X", "X")
    # depth grid: kept from max(2, dmin_thres) upwards, whatever singleton the reads left
    dg = fam("depth-grid")
    assert sorted({c.tags["depth"] for c in dg}) == sorted(G.GRID_DEPTHS)
    for c in dg:
        assert (c.result(dmin_thres) is not None) == (c.tags["depth"] >= floor), c.name
        if c.result(dmin_thres):
            assert c.result(dmin_thres)[0] == c.tags["depth"]
    assert {c.result(dmin_thres)[0] for c in dg if c.result(dmin_thres)} >= {20, 65534, 65535}
    # a depth in [2, dmin_thres) is what a literal 2 would keep
    assert any(2 <= c.tags["depth"] < dmin_thres for c in dg) == (dmin_thres > 2)
    # several occurrences with the same extensions: the smallest depth decides, in both orders
    se = {c.name: c for c in fam("same-exts")}
    for name in ("depths 5, 2 ++", "depths 2, 5 ++", "depths 5, 2 +-", "depths 2, 5 --"):
        assert se[name].result(dmin_thres) == ((2,) + se[name].ctg_result(1)[1:] if dmin_thres <= 2 else None)
    assert se["depths 65535, 65534 +-"].result(dmin_thres)[0] == 65534
    assert all(c.result(dmin_thres) is None for c in se.values() if min(c.tags["depths"]) < floor)
    assert all(c.result(dmin_thres)[0] == min(c.tags["depths"]) for c in se.values() if min(c.tags["depths"]) >= floor)
    assert any(len(c.occs) == 3 and c.result(dmin_thres) for c in se.values())
    # one occurrence differs, has an N or a lower-case neighbour: absent
    df = fam("differs")
    assert {c.tags["what"] for c in df} == {"other", "N", "lower"} and all(c.result(dmin_thres) is None for c in df)
    assert any("N" in s[0] + s[-1] for c in df for s, _ in c.contigs()) and any((s[0] + s[-1]).upper() != s[0] + s[-1] for c in df for s, _ in c.contigs())
    assert any(len({w[0] for w in c.windows()}) == 2 and len({w[1] for w in c.windows()}) == 1 for c in df)  # a different left
    assert any(len({w[0] for w in c.windows()}) == 1 and len({w[1] for w in c.windows()}) == 2 for c in df)  # a different right
    # one on each strand: kept with the smaller depth when consistent; the inconsistent ones are shown with equal letters
    for c in fam("strands"):
        assert {o[3] for o in c.occs} == {"+", "-"}
        assert (c.result(dmin_thres) is not None) == (c.tags["consistent"] and min(o[2] for o in c.occs) >= floor), c.name
        if not c.tags["consistent"]:
            (s1, _), (s2, _) = c.contigs()
            assert (s1[0], s1[-1]) == (s2[0], s2[-1]) and len({w[:2] for w in c.windows()}) == 2
    assert any(c.result(dmin_thres) for c in fam("strands"))
    # the larger strand only: the result carries the swapped sides
    ls = fam("larger-strand")
    assert ls and all(c.orient == "given" and G.revcomp(c.kmer) < c.kmer for c in ls)
    first = ls[0]
    assert first.result(dmin_thres) == (9, "G", "T") and first.contigs()[0][0][0] + first.contigs()[0][0][-1] == "AC"
    assert any(c.result(dmin_thres) == c.reads.result(dmin_thres) != None for c in ls)  # noqa: E711
    # inside K
    ins = fam("inside")
    assert any("N" in s[1:-1] for c in ins for s, _ in c.contigs()) and any(s[1:-1] != s[1:-1].upper() for c in ins for s, _ in c.contigs())
    assert all(c.result(dmin_thres) == (min(o[2] for o in c.occs),) + c.windows()[0][:2] for c in ins)
    assert any(len(c.occs) == 2 and c.spell == ["N", None] for c in ins)
    # k + 1 characters
    sh = fam("short")
    assert all(any(len(s) == k + 1 for s, _ in c.contigs()) for c in sh)
    assert all((c.result(dmin_thres) is not None) == c.tags["kept"] for c in sh)
    # palindromes only at even k
    pal = fam("palindrome")
    assert bool(pal) == (k % 2 == 0)
    for c in pal:
        assert G.revcomp(c.kmer) == c.kmer
        assert (c.result(dmin_thres) is not None) == (c.tags["kept"] and min(o[2] for o in c.occs) >= floor), c.name
    if pal:
        alone = {c.name: c for c in pal}
        assert alone["palindrome, forward alone"].result(dmin_thres) == (9, "A", "C")
        assert alone["palindrome, other strand alone"].result(dmin_thres) == (9, "G", "T")  # what is shown, not swapped back
    # the emitter: every contig has k + 2 characters (or k + 1), the block is the contigs joined, depths lie under every byte
    ctgs, depths = G.emit_ctgs(cases, seed=3)
    block, dd = G.as_block(ctgs, depths)
    assert sorted(zip(ctgs, depths)) == sorted(zip(*G.emit_ctgs(cases)))
    assert block.tobytes().decode() == "_".join(ctgs) + "_" and len(dd) == len(block) and dd.dtype == np.uint16
    at = 0
    for s, d in zip(ctgs, depths):
        assert k + 1 <= len(s) <= k + 2 and (dd[at:at + len(s) + 1] == d).all()
        at += len(s) + 1
    distinct, positions = G.expected_ctg_stats(cases)
    assert positions == len(block) and distinct == len(cases) - sum(1 for c in sh if not c.windows())
