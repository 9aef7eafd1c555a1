"""tests/count_cases.py against the two restatements: the entries and results a family expects by construction equal
spec_model.count_kmers' and the C oracle's, and every family holds the cases it is for.  No GPU."""
import pytest

import count_cases as CC
import spec_model
from oracle import cpu_oracle as O

KS = [5, 21, 33, 77]


def family_blocks(cases, k, seed):
    nblocks = max(len(c.blocks) for c in cases)
    return [CC.emit(cases, k, seed + 100 * b, block=b) for b in range(nblocks)]


def check_against_both(cases, k, dmin_thres, seed=11):
    blocks = family_blocks(cases, k, seed)
    nreads = sum(len(b[2]) - 1 for b in blocks)
    assert nreads == sum(c.occurrences for c in cases)
    ekeys, ecounts, eexts = CC.expected_table(cases)
    rkeys, rcounts, rleft, rright = CC.expected_results(cases, dmin_thres)
    est = CC.expected_stats(cases, dmin_thres)
    # the C oracle
    o = O.Oracle(k, dmin_thres=dmin_thres, nranks=3, nthreads=2)
    for b, q, offs in blocks:
        o.add_reads(b, q, offs)
    okeys, ocounts, oexts = o.dump_table()
    ores = o.finalize()
    ost = o.stats()
    o.close()
    assert okeys.shape == ekeys.shape and (okeys == ekeys).all()
    bad = [c.name for c, a, b_, x, y in zip(sorted(cases, key=lambda c: c.key), ocounts, ecounts, oexts, eexts) if a != b_ or (x != y).any()]
    assert not bad, bad
    for got, want, name in zip(ores, (rkeys, rcounts, rleft, rright), ("keys", "counts", "left", "right")):
        assert got.shape == want.shape and (got == want).all(), name
    assert ost["dropped"] == 0
    assert (ost["unique"], ost["purged"], ost["total_kmers"], ost["sum_counts"], ost["kmers_inserted"]) == (
        est["num_unique"], est["num_purged"], est["total_kmers"], est["sum_counts"], est["kmers_inserted"])
    assert ost["raw_kmers"] == 3 * nreads  # a read of k + 2 bases has three k-mers, one of them with both neighbours
    for i in range(0, len(ekeys), 17):  # the packing is the oracle's
        c = sorted(cases, key=lambda c: c.key)[i]
        assert (O.pack_kmer(c.canon) == ekeys[i]).all()
    # the second restatement
    reads, quals = [], []
    for b, q, _ in blocks:
        r, ql = CC.read_strings(b, q, k)
        reads += r
        quals += ql
    mres, mtable = spec_model.count_kmers(reads, quals, k, dmin_thres=dmin_thres)
    assert len(mtable) == len(ekeys)
    for c in cases:
        assert mtable[c.canon] == [c.count, c.lc, c.rc], c.name
    assert mres == sorted((c.canon,) + c.result(dmin_thres) for c in cases if c.result(dmin_thres))
    lines = sorted(c.line(dmin_thres) for c in cases if c.result(dmin_thres))
    assert lines == ["%s %d %s %s" % r for r in mres]


@pytest.mark.parametrize("dmin_thres", [1, 2, 3, 5])
@pytest.mark.parametrize("k", KS)
def test_vote_grid_matches_model_and_oracle(k, dmin_thres):
    cases = CC.vote_grid(k, dmin_thres)
    assert len({c.key for c in cases}) == len(cases)
    check_against_both(cases, k, dmin_thres)


@pytest.mark.parametrize("dmin_thres", [1, 2, 3, 5])
def test_vote_grid_holds_what_it_is_for(dmin_thres):
    cases = CC.vote_grid(21, dmin_thres)
    for c in (30, 40, 50, 100):
        at = [cs for cs in cases if cs.tags["c"] == c and cs.count == c]
        exts = [cs.exts(dmin_thres) for cs in at]
        assert any(cs.result(dmin_thres) for cs in at), c
        assert any("X" in e for e in exts) and any("F" in e for e in exts), c
    # the threshold in double is not count / 10: at least one outcome changes with the integer threshold
    changed = 0
    for cs in cases:
        naive = max(cs.count // 10, dmin_thres)
        for c4 in (cs.lc, cs.rc):
            top, runner = sorted(c4, reverse=True)[:2]
            changed += ("X" if top < naive else "F" if runner >= naive else "U") != ("X" if top < cs.tags["d"] else "F" if runner >= cs.tags["d"] else "U")
    assert changed >= 1
    assert CC.dmin_dyn(30, 2) == 2 and CC.dmin_dyn(40, 2) == 3 and CC.dmin_dyn(50, 2) == 4 and CC.dmin_dyn(100, 2) == 9
    # the swap of sides decides the larger-strand cases: as given, their sides vote differently
    larger = [cs for cs in cases if cs.tags["kind"] == "larger-strand"]
    assert larger and all(cs.swapped and cs.orient == "given" for cs in larger)
    assert any(cs.exts(dmin_thres)[0] != cs.exts(dmin_thres)[1] for cs in larger)
    # every top letter and every runner letter occurs
    assert {cs.lc.index(max(cs.lc)) for cs in cases if max(cs.lc)} == {0, 1, 2, 3}
    assert {cs.rc.index(max(cs.rc)) for cs in cases if max(cs.rc)} == {0, 1, 2, 3}


@pytest.mark.parametrize("k", KS)
def test_saturation_matches_model_and_oracle(k):
    cases = CC.saturation(k)
    check_against_both(cases, k, 2)
    assert len(cases) == 20 and max(c.occurrences for c in cases) == 70000
    # a half at 65534 beside 1, at 65535 beside 1, and both "none" halves full
    assert any(sorted(c.lc)[-2:] == [1, 65534] and sorted(c.rc)[-2:] == [1, 65534] for c in cases)
    assert any(sorted(c.lc)[-2:] == [1, 65535] for c in cases)
    assert any(c.count == 65535 and max(c.lc) == 0 and max(c.rc) == 0 for c in cases)
    kept = [c for c in cases if c.result(2)]
    assert len(kept) == 10 and all(c.tags["split"] in (0, 1) for c in kept)


@pytest.mark.parametrize("n", [65535, 65536])
@pytest.mark.parametrize("k", KS)
def test_region_fill_matches_model_and_oracle(k, n):
    cases = CC.region_fill(k, n)
    assert sum(c.occurrences for c in cases) == n and max(c.occurrences for c in cases) < 65535
    check_against_both(cases, k, 2)


@pytest.mark.parametrize("k", KS)
def test_two_pass_matches_model_and_oracle(k):
    cases = CC.two_pass(k)
    check_against_both(cases, k, 2)
    by = {c.name: c for c in cases}
    assert by["1+1"].result(2) == (2, by["1+1"].exts(2)[0], by["1+1"].exts(2)[1]) and by["1+1"].exts(2)[0] in "ACGT"
    assert by["1+0"].result(2) is None and by["0+1"].result(2) is None
    assert by["32767+32768"].count == 65535 and by["32767+32768"].occurrences == 65535
    assert sorted(by["40000+40000 left A then C"].lc)[-2:] == [40000, 40000] and by["40000+40000 left A then C"].count == 65535
    assert by["65535+1"].count == 65535 and sorted(by["65535+1"].lc + by["65535+1"].rc)[-3:] == [1, 65535, 65535]
    c = by["30+10 runner 3 in the second"]
    assert c.count == 40 and CC.dmin_dyn(40, 2) == 3 and "F" in c.exts(2)
