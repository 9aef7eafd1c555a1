"""tests/lassm_model.py against cases whose answer follows from the case alone (no GPU needed): the model is the
definition kc_local_assm is compared with, so it is held against hand-built ends first."""
import numpy as np
import pytest

import depth_model as D
import lassm_cases as LC
import lassm_model as M
from align_model import revcomp


def right(out, u=0):
    block, offsets, ends, st = out
    e = ends[2 * u + 1]
    ctg = LC.new_contigs(block, offsets)[u]
    return ctg[len(ctg) - int(e["ext_len"]):] if e["ext_len"] else "", int(e["status"]), int(e["iters"]), int(e["mer_len"])


def test_two_copies_extend_by_the_overhang_and_one_copy_by_nothing():
    c, G = LC.overhang_case(2)
    assert right(c.model()) == (G[200:300], M.DEAD_END, 2, 13)
    block, offsets, ends, st = c.model()
    assert LC.new_contigs(block, offsets) == [G[:300]] and list(offsets) == [0, 301]
    assert tuple(ends[0]) == (0, 0, 0, 0, 0, M.NO_CANDS) and tuple(ends[1]) == (2, 100, 200, 2, 13, M.DEAD_END)
    assert st == {"ends": 2, "status": [1, 0, 1, 0, 0, 0], "cands_overhang": 2, "cands_mate": 0, "cand_bases": 280, "iterations": 2,
                  "ext_bases": 100, "ctgs_extended": 1}
    c, G = LC.overhang_case(1)
    assert right(c.model()) == ("", M.DEAD_END, 2, 13)


def test_haplotypes_fork_after_every_upward_shift():
    c, G = LC.haplotype_case()
    assert right(c.model(max_mer_len=61)) == (G[200:250], M.FORK, 6, 61)


def test_short_repeat_is_walked_through_after_one_shift_and_a_long_one_is_not():
    c, V = LC.repeat_case(25)
    assert right(c.model(max_mer_len=61)) == (V, M.DEAD_END, 2, 29)  # the direction lock: no shift down after the shift up
    c, V = LC.repeat_case(70)
    assert right(c.model(max_mer_len=61)) == ("", M.FORK, 6, 61)


def test_short_overlap_is_rescued_by_the_downward_shift():
    c, G = LC.overhang_case(2, start=185, stop=285)
    assert right(c.model()) == (G[200:285], M.DEAD_END, 2, 13)
    assert right(c.model(min_mer_len=21)) == ("", M.DEAD_END, 1, 21)


def test_tandem_repeat_loops():
    c, unit = LC.tandem_case()
    assert right(c.model()) == (unit, M.LOOP, 1, 21)


@pytest.mark.parametrize("q0,q1,extends", [(20, 10, True), (19, 19, False), (20, 9, False), (20, 20, True), (10, 10, False)])
def test_viability_needs_the_threshold_and_one_high_quality_base(q0, q1, extends):
    G = LC.genome(1, 350)
    c = LC.Case([G[:200]])
    for q in (q0, q1):  # only the first base beyond the contig differs in quality
        c.pair(G[160:300], 0, 160, qual="I" * 40 + chr(33 + q) + "I" * 99)
    ext, status, iters, m = right(c.model())
    assert (ext, status) == ((G[200:300] if extends else ""), M.DEAD_END)


def test_threshold_from_the_depth():
    for copies, want in ((4, 0), (5, 100)):
        c, G = LC.overhang_case(copies)
        c.means = [25]  # thr = 200 * 25 / 1000 = 5
        assert len(right(c.model())[0]) == want
        c.means = [24]  # 4
        assert len(right(c.model())[0]) == 100
    c, G = LC.overhang_case(2)
    assert len(right(c.model(min_viable=3))[0]) == 0


def test_max_walk_len_is_reached_exactly():
    c, G = LC.overhang_case(2)
    assert right(c.model(max_walk_len=100)) == (G[200:300], M.MAX_LEN, 1, 21)
    assert right(c.model(max_walk_len=99)) == (G[200:299], M.MAX_LEN, 1, 21)
    assert right(c.model(max_walk_len=101)) == (G[200:300], M.DEAD_END, 2, 13)
    assert right(c.model(max_walk_len=1)) == (G[200], M.MAX_LEN, 1, 21)


def test_contig_shorter_than_the_shortest_mer():
    G = LC.genome(1, 300)
    c = LC.Case([G[100:110]])
    for _ in range(2):
        c.pair(G[50:200], 0, -50)
    block, offsets, ends, st = c.model()
    assert [tuple(e)[1:] for e in ends] == [(0, 0, 2, 13, M.DEAD_END), (0, 10, 2, 13, M.DEAD_END)] and [int(e["cands"]) for e in ends] == [2, 2]
    assert bytes(block) == (G[100:110] + "_").encode()


def cands_of(c, **kw):
    return [int(e["cands"]) for e in c.model(**kw)[2]]


def test_overhang_rules_at_their_boundaries():
    G = LC.genome(1, 400)
    for orient in (0, 1):
        for pos, want in ((100, [0, 0]), (101, [0, 1]), (0, [0, 0]), (-1, [1, 0])):  # pe = len_u, len_u + 1; ps = 0, -1
            c = LC.Case([G[100:300]])
            c.pair(G[100 + pos:200 + pos], 0, pos, orient, mate="", mate_at=None)
            assert cands_of(c) == want, (orient, pos)
    c = LC.Case([G[100:150]])
    c.pair(G[90:160], 0, -10)  # over both ends
    assert cands_of(c) == [1, 1]


def test_mate_rules_at_their_boundaries_and_placements():
    G = LC.genome(1, 400)
    mate = LC.genome(2, 80)
    # orient 0: ps + max_insert = len_u and len_u + 1 (ps = 50, len_u = 200)
    for max_insert, want in ((150, [0, 0]), (151, [0, 1])):
        c = LC.Case([G[100:300], G[320:400]])
        c.pair(G[150:250], 0, 50, 0, mate=mate)
        assert cands_of(c, max_insert=max_insert)[:2] == want
    # orient 1: pe - max_insert = 0 and -1 (pe = 150)
    for max_insert, want in ((150, [0, 0]), (151, [1, 0])):
        c = LC.Case([G[100:300], G[320:400]])
        c.pair(G[150:250], 0, 50, 1, mate=mate)
        assert cands_of(c, max_insert=max_insert)[:2] == want
    # the mate placed on u, on another contig, unplaced, empty
    for mate_at, text, want in (((0, 100, 1), mate, 0), ((1, 0, 1), mate, 1), (None, mate, 1), (None, "", 0)):
        c = LC.Case([G[100:300], G[320:400]])
        c.pair(G[150:250], 0, 50, 0, mate=text, mate_at=mate_at)
        assert cands_of(c)[1] == want, mate_at
    # the candidate text is the mate's reverse complement, at either end
    c = LC.Case([G[100:300]])
    c.pair(G[150:250], 0, 50, 0, mate="ACCGT" * 4)
    alns, pairs, quals = c.arrays()
    ends = M.candidates(c.contigs, c.reads, quals, alns, pairs, dict(M.DEFAULTS), 33)
    assert [len(e) for e in ends] == [0, 1] and ends[1][0][0] == M.codes_of(revcomp("ACCGT" * 4)) and ends[1][0][2] is True


def test_a_read_gives_at_most_three_candidates_and_too_many_is_refused_per_end():
    G = LC.genome(1, 400)
    c = LC.Case([G[100:150]])
    c.pair(G[90:160], 0, -10, 0, mate=LC.genome(3, 50))
    assert cands_of(c) == [1, 2]
    c, G = LC.overhang_case(3)
    assert tuple(c.model(max_cands=2)[2][1]) == (3, 0, 200, 0, 0, M.TOO_MANY)
    assert int(c.model(max_cands=3)[2][1]["ext_len"]) == 100


def test_n_and_lower_case():
    c, G = LC.overhang_case(2)
    c.reads[0] = c.reads[0][:60] + "N" + c.reads[0][61:]          # one copy loses the windows over the N and the N as a base
    assert right(c.model())[0] == G[200:220]                     # support drops to one where the N is the extension base
    c, G = LC.overhang_case(2)
    c.reads[0] = c.reads[0].lower()
    assert right(c.model())[0] == G[200:300]
    c, G = LC.overhang_case(2)
    c.contigs[0] = c.contigs[0][:190] + "N" + c.contigs[0][191:]  # N in the tail
    assert right(c.model())[0] == ""                              # the mer at 13 holds positions 187..199, the N among them
    c.contigs[0] = G[:185] + "N" + G[186:200]
    assert right(c.model()) == (G[200:300], M.DEAD_END, 2, 13)    # 187..199 is clear of it


def test_errors():
    c, G = LC.overhang_case(2)
    alns, pairs, quals = c.arrays()
    for bad in (dict(min_mer_len=3), dict(max_mer_len=129), dict(min_mer_len=30, max_mer_len=29), dict(shift=0), dict(shift=65),
                dict(max_walk_len=0), dict(max_walk_len=4097), dict(max_insert=0), dict(max_insert=65536), dict(min_qual=21),
                dict(hi_qual=94), dict(min_viable=0), dict(viable_permille=1001), dict(max_cands=0), dict(max_cands=(1 << 20) + 1),
                dict(flags=1)):
        with pytest.raises(D.BadArg):
            c.model(**bad)
    with pytest.raises(D.BadArg):
        M.local_assm(c.contigs, c.reads[:3], None, alns, pairs)
    for field, value in (("aln0", 7), ("aln1", 0), ("aln0", 0)):
        p = pairs.copy()
        p[1][field] = value
        with pytest.raises(M.BadPair) as e:
            M.local_assm(c.contigs, c.reads, None, alns, p)
        assert e.value.index == 1
    a = alns.copy()
    a[1]["kind"] = M.KIND_NONE
    with pytest.raises(M.BadPair):
        M.local_assm(c.contigs, c.reads, None, a, pairs)
    a = alns.copy()
    a[1]["rstop"] = 141
    with pytest.raises(D.BadRecord):
        M.local_assm(c.contigs, c.reads, None, a, pairs)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mirror_property(seed):
    c = LC.random_case(seed, pairs=80)
    block, offsets, ends, st = c.model(k=15, min_mer_len=7, max_walk_len=60)
    mblock, moffsets, mends, mst = c.mirrored().model(k=15, min_mer_len=7, max_walk_len=60)
    assert st["ext_bases"] > 0 and st == mst
    assert LC.new_contigs(mblock, moffsets) == [revcomp(s) for s in LC.new_contigs(block, offsets)]
    for u in range(len(c.contigs)):
        for f in ("cands", "ext_len", "iters", "mer_len", "status"):
            assert int(ends[2 * u][f]) == int(mends[2 * u + 1][f]) and int(ends[2 * u + 1][f]) == int(mends[2 * u][f])
    assert (np.diff(offsets.astype(np.int64)) == np.diff(moffsets.astype(np.int64))).all()
