"""tests/correct_model.py, the model the device tests of kc_correct_reads compare with, held to what follows from the
constructions of tests/correct_cases.py alone: planted substitutions come back, the fix list is the plan, every reason a run
or a site can be left with is produced, and the seeds chosen here exercise both sides, runs with both sites and more than one
round -- the device tests inherit them.  No GPU needed."""
import numpy as np
import pytest

import correct_cases as CC
import correct_model as M
import kdepth_model as K

KS = (21, 33, 64)


def run(k, reads, quals=None, **kw):
    tab = CC.counted(k)[4]
    b, offs = K.block(reads)
    return M.correct_reads(tab, k, b, offs, quals=quals, **kw)


@pytest.mark.parametrize("k", KS)
def test_the_counted_genome_is_solid_and_the_fork_is_there(k):
    G, (p1, p2), _, _, tab = CC.counted(k)
    counts = [tab.get(K.canonical(G[p:p + k]), 0) for p in range(len(G) - k + 1)]
    assert counts[0] == 0 and counts[-1] == 0 and min(counts[1:-1]) >= 2  # the two ends have a dead end
    assert G[p1:p1 + k - 1] == G[p2:p2 + k - 1] and G[p1 + k - 1] != G[p2 + k - 1] and G[p1 - 1] != G[p2 - 1]
    out, recs, fixes, stats = run(k, [G[5:400], K.revcomp(G[300:800]), G[5:400].lower()])
    assert (out == K.block([G[5:400], K.revcomp(G[300:800]), G[5:400].lower()])[0]).all() and len(fixes) == 0
    assert stats == dict(seqs=3, bytes=395 * 2 + 500, windows=2 * (396 - k) + 501 - k, weak_before=0, weak_after=0, sites=0, accepted=0, rounds=1)
    assert not recs["flags"].any() and not recs["weak_before"].any()


@pytest.mark.parametrize("k", KS)
def test_planted_errors_come_back_and_the_fixes_are_the_plan(k):
    cases = CC.planted_cases(k)
    assert len(cases) == 5 + 7 + 3 + 6
    out, recs, fixes, stats = run(k, [c[1] for c in cases], min_windows=1)
    offs = K.block([c[1] for c in cases])[1]
    for i, (name, read, want, plan, why) in enumerate(cases):
        a, b = int(offs[i]), int(offs[i + 1])
        assert out[a:b].tobytes() == want, name
        mine = fixes[fixes["seq"] == i]
        assert sorted((int(f["pos"]), int(f["old"]), int(f["new"])) for f in mine) == plan, name
        assert recs[i]["corrected"] == len(plan) and recs[i]["flags"] == why, (name, recs[i])
        if want != read:
            assert recs[i]["weak_after"] == 0 and recs[i]["weak_before"] > 0, name
        # each case alone gives what it gives in the block: sequences do not see each other
        alone = run(k, [read], min_windows=1)
        assert alone[0].tobytes() == want and alone[1][0]["flags"] == why, name
    assert stats["accepted"] == len(fixes) == sum(len(c[3]) for c in cases) and stats["rounds"] == 3
    assert (np.diff([(int(f["round"]) << 40) + (int(f["seq"]) << 20) + int(f["pos"]) for f in fixes]) > 0).all()  # (round, seq, pos)


@pytest.mark.parametrize("k", KS)
def test_the_seeds_reach_both_sides_both_sites_and_a_second_round(k):
    cases = CC.planted_cases(k)
    names = [c[0] for c in cases]
    out, recs, fixes, stats = run(k, [c[1] for c in cases], min_windows=1)
    assert set(fixes["side"]) == {M.LEFT, M.RIGHT} and set(fixes["round"]) == {1, 2}
    both = fixes[fixes["seq"] == names.index("two errors %d apart" % k)]  # a run of 2k windows: its two sites in one round
    assert [(int(f["round"]), int(f["side"]), int(f["score"]), int(f["runner_up"])) for f in both] == [(1, M.LEFT, k, 0), (1, M.RIGHT, k, 0)]
    later = fixes[fixes["seq"] == names.index("two errors %d apart" % CC.MIN_GAIN)]  # k + 8 windows: the left site, then what is left
    assert [(int(f["round"]), int(f["side"]), int(f["score"])) for f in later] == [(1, M.LEFT, CC.MIN_GAIN), (2, M.LEFT, k)]
    first = fixes[fixes["seq"] == names.index("one error: first")]
    assert [(int(f["pos"]), int(f["side"]), int(f["score"])) for f in first] == [(0, M.RIGHT, 1)]
    # rounds = 1 stops there: the second error of the pair stays, and the record says how many weak windows with it
    one = run(k, [c[1] for c in cases], min_windows=1, rounds=1)
    i = names.index("two errors %d apart" % CC.MIN_GAIN)
    assert one[3]["rounds"] == 1 and one[1][i]["corrected"] == 1 and one[1][i]["weak_after"] == k and len(one[2]) == (fixes["round"] == 1).sum()


@pytest.mark.parametrize("k", KS)
def test_every_reason_is_produced(k):
    for name, read, quals, kw, why in CC.verdict_cases(k):
        out, recs, fixes, stats = run(k, [read], quals=quals, **kw)
        assert out.tobytes() == read and len(fixes) == 0 and recs[0]["flags"] == why, (name, recs[0])
        assert recs[0]["weak_before"] == recs[0]["weak_after"] > 0 and stats["rounds"] == 1
        assert stats["sites"] == (1 if why in (M.AMBIGUOUS, M.NO_GAIN) else 0), name
    # the gates are the only thing in the way of the last two
    name, read, quals, kw, why = CC.verdict_cases(k)[4]
    assert run(k, [read], min_windows=1)[3]["accepted"] == 1
    name, read, quals, kw, why = CC.verdict_cases(k)[5]
    assert run(k, [read], quals=quals, min_windows=1, max_qual=30)[3]["accepted"] == 1 and run(k, [read], min_windows=1, max_qual=20)[3]["accepted"] == 1


def test_nothing_and_small_rules():
    k = 5
    tab = {K.canonical(w): 3 for w in (b"AACCG", b"ACCGT", b"CCGTA", b"CGTAG", b"GTAGA")}
    # AACCGTAGA with its fifth byte wrong: windows 0 .. 4 hold it, no anchor on either side
    out, recs, fixes, stats = M.correct_reads(tab, k, *K.block([b"AACCTTAGA"]), min_windows=1)
    assert out.tobytes() == b"AACCTTAGA" and recs[0]["flags"] == M.UNANCHORED and stats["windows"] == 5 and stats["weak_before"] == 5
    # ... its last byte wrong: one weak window, anchored on the left; lower case stays lower case
    out, recs, fixes, stats = M.correct_reads(tab, k, *K.block([b"AACCGTAGc", b"", b"AACC"]), min_windows=1)
    assert out.tobytes() == b"AACCGTAGaAACC" and [tuple(f) for f in fixes] == [(0, 8, ord("c"), ord("a"), 1, M.LEFT, 1, 0)]
    assert stats == dict(seqs=3, bytes=13, windows=5, weak_before=1, weak_after=0, sites=1, accepted=1, rounds=2)
    empty = M.correct_reads(tab, k, *K.block([]))
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and len(empty[2]) == 0 and empty[3] == dict.fromkeys(M.STATS, 0)
    assert M.REC_DTYPE.itemsize == 16 and M.FIX_DTYPE.itemsize == 16


@pytest.mark.parametrize("seed", (32, 82))  # tests/test_chain_model.py's SEEDS
def test_the_model_chain_on_noisy_reads_shrinks_the_table_and_the_dynamic_programme(seed):
    """tests/chain_cases.py's noisy pairs counted, corrected and counted again, then aligned before and after: the table holds
    fewer k-mers (its entries before the purge: the wrong k-mers were nearly all singletons, so the results do not shrink; they
    gain the few true k-mers whose second sighting the correction supplies) and a smaller share of the gapped records needs
    the dynamic programme.  The device chain (tests/test_gpu_correct_chain.py) asserts the same two inequalities."""
    import align_model as A
    import chain_cases as NC
    import gap_model as GM
    from oracle import cpu_oracle as O
    case = NC.noisy_assembly(seed)
    k = NC.K
    (keys, counts, _, _), st = O.count_reads(case.reads, case.quals, k=k)
    b, offs = K.block(case.reads)
    out, recs, fixes, stats = M.correct_reads(K.table(keys, counts, k), k, b, offs)
    fixed = [out[int(offs[i]):int(offs[i + 1])].tobytes().decode() for i in range(len(offs) - 1)]
    assert stats["accepted"] > 500 and stats["weak_after"] < stats["weak_before"] // 4
    (keys2, _, _, _), st2 = O.count_reads(fixed, case.quals, k=k)
    assert st2["unique"] < st["unique"] // 2 and len(keys) <= len(keys2) <= len(keys) + 100
    sub = case.subset(100)
    index = A.Index(*A.join_block(sub.contigs), k)
    share = []
    for reads in (sub.reads, fixed[:200]):
        gst = GM.align_gapped(sub.contigs, reads, A.align_reads(index, reads)[0])[1]
        share.append(gst["dp"] / gst["records"])
    assert share[1] < share[0] / 2
