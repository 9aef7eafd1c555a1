"""tests/close_model.py against cases whose answer follows from the case alone (no device, no aligner)."""
import numpy as np
import pytest

import close_cases as CC
import close_model as M
import depth_model as D
import links_cases as LC
import scaffold_model as SM
import test_scaffold_model as TS
from close_cases import hand_case, revc, two_contigs
from depth_model import rec, records


def run(case, **kw):
    res = M.close_gaps(*case.args(), **kw)
    check_shape(case, res)
    return res


def closure(res, m=1):
    c = res[4][m]
    return dict(status=int(c["status"]), cands=int(c["cands"]), reads=int(c["reads"]), old=int(c["old_join"]), new=int(c["new_join"]),
                disputed=int(c["disputed"]), fill_pos=int(c["fill_pos"]))


def check_shape(case, res):
    """what holds for every result: the identities of the statistics, the records against the text"""
    seqs, offsets, scafs, members, closures, st = res
    n = len(case.contigs)
    assert st["gaps"] == st["gaps_no_reads"] + st["gaps_weak"] + st["filled"] + st["abutted"] + st["overlapped"] + st["overlaps_rejected"]
    assert st["members"] == n == len(members) == len(closures) and st["joins"] == n - len(scafs)
    assert len(offsets) == len(scafs) + 1 and int(offsets[-1]) == len(seqs) and seqs.count(b"_") == len(scafs)
    assert st["n_bases_left"] == sum(int(s["n_bases"]) for s in scafs) and st["disputed_cols"] == sum(int(c["disputed"]) for c in closures)
    assert st["fill_bases"] == sum(int(c["new_join"]) for c in closures if c["status"] == M.FILLED)
    for s in range(len(scafs)):
        assert int(offsets[s + 1]) - int(offsets[s]) - 1 == int(scafs[s]["len"]) and seqs[int(offsets[s + 1]) - 1:int(offsets[s + 1])] == b"_"
        assert int(scafs[s]["flags"]) == int(case.scaffolds[s]["flags"])
    for m in range(n):
        x, c = members[m], closures[m]
        t = SM.node_text(case.contigs, 2 * int(x["ctg"]) + int(x["orient"])).encode()
        j = int(x["join"])
        assert j == int(c["new_join"]) and int(c["old_join"]) == int(case.members[m]["join"])
        assert seqs[int(x["out_pos"]):int(x["out_pos"]) + len(t) - max(-j, 0)] == t[max(-j, 0):]
        if c["status"] in (M.NO_READS, M.WEAK, M.OVERLAP_REJECTED):
            assert j == int(c["old_join"]) > 0 and seqs[int(c["fill_pos"]):int(c["fill_pos"]) + j] == b"N" * j
        if c["status"] == M.FILLED:
            assert int(c["fill_pos"]) + j == int(x["out_pos"]) and j > 0


# ---- two contigs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 7, 63, 64, 65])
@pytest.mark.parametrize("oa,ob", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_two_contigs_in_all_four_orientation_pairs(g, oa, ob):
    case = two_contigs(g, oa, ob, old_join=20)
    res = run(case)
    assert M.strings(res) == [case.text]
    assert closure(res) == dict(status=M.FILLED, cands=3, reads=3, old=20, new=g, disputed=0, fill_pos=60)
    assert res[5]["filled"] == 1 and res[5]["fill_bases"] == g and res[5]["n_bases_left"] == 0 and res[5]["cands_off_join"] == 0
    # the scaffold read from its other end: B' then A', the forward supporters are the backward ones now
    case2 = CC.build(revc(case.text), [(0, 70, ob ^ 1), (70 + g, 130 + g, oa ^ 1)], [(len(case.text) - e, len(case.text) - s, r ^ 1)
                                                                                      for s, e, r in [(30, 90 + g, 0)] * 2 + [(30, 90 + g, 1)]],
                     order=(1, 0))
    assert case2.contigs == case.contigs and case2.reads == case.reads
    assert M.strings(run(case2)) == [revc(case.text)]


@pytest.mark.parametrize("seed", [1, 2])
def test_reverse_complements_and_shuffled_numbers(seed):
    a, b = CC.chain(9, seed=seed), CC.chain(9, seed=seed, flip=True, reorder=seed + 50)
    ra, rb = run(a), run(b)
    assert M.strings(ra) == M.strings(rb) == [a.text]
    assert [revc(c) for c in a.contigs] != b.contigs and sorted(revc(c) for c in a.contigs) == sorted(b.contigs)
    assert ra[5]["filled"] == rb[5]["filled"] == 8 and ra[5]["n_bases_left"] == 0


def test_records_that_stop_short_of_the_end_within_the_slack():
    case = two_contigs(7)
    for x in case.alns:
        if x["ctg"] == 0:
            x["cstop"] -= 3
            x["rstop"] -= 3
        else:
            x["cstart"] += 3
            x["rstart"] += 3
    assert M.strings(run(case)) == [case.text]
    res = run(case, end_slack=2)  # no record reaches its end any more
    assert closure(res)["status"] == M.NO_READS and res[5]["cands"] == 0


def test_min_reads_at_the_threshold_and_one_under():
    case = two_contigs(7, old_join=4)
    assert closure(run(case, min_reads=3))["status"] == M.FILLED
    res = run(case, min_reads=4)
    assert closure(res) == dict(status=M.WEAK, cands=3, reads=0, old=4, new=4, disputed=0, fill_pos=60)
    assert M.strings(res) == [case.text[:60] + "NNNN" + case.text[67:]] and res[5]["n_bases_left"] == 4 and res[5]["gaps_weak"] == 1


A60, B70 = CC.rand_seq(np.random.default_rng(7), 60), CC.rand_seq(np.random.default_rng(8), 70)


def test_min_agree_permille_at_the_threshold_and_one_over():
    case = hand_case(A60, B70, ["ACG", "ACG", "ACG", "ACGTT"])
    assert closure(run(case, min_agree_permille=750)) == dict(status=M.FILLED, cands=4, reads=3, old=9, new=3, disputed=0, fill_pos=60)
    assert closure(run(case, min_agree_permille=751))["status"] == M.WEAK


def test_the_gap_mode_a_tie_goes_to_the_smaller_gap_and_a_minority_length_is_ignored():
    res = run(hand_case(A60, B70, ["TTTTT", "ACG", "TTTTT", "ACG"]), min_agree_permille=500)
    assert M.strings(res) == [A60 + "ACG" + B70] and closure(res)["reads"] == 2 and closure(res)["disputed"] == 0
    res = run(hand_case(A60, B70, ["ACG", "TTTTT", "ACG", "ACG", "GGGGGGG"], backward=(1, 2)))
    assert M.strings(res) == [A60 + "ACG" + B70] and closure(res)["reads"] == 3 and closure(res)["cands"] == 5


def test_column_votes():
    # ties go to A before C before G before T; lower case votes; N and other bytes do not; an all-N column is N
    res = run(hand_case(A60, B70, ["TGCA", "ACGT"]))
    assert M.strings(res) == [A60 + "ACCA" + B70] and closure(res)["disputed"] == 4
    res = run(hand_case(A60, B70, ["gNNt-", "gNNCc", "TNNtc"], backward=(2,)))
    assert M.strings(res) == [A60 + "GNNTC" + B70] and closure(res)["disputed"] == 2
    res = run(hand_case(A60, B70, ["NN", "N*"], backward=(0,)))
    assert M.strings(res) == [A60 + "NN" + B70] and closure(res)["disputed"] == 0 and res[5]["fill_bases"] == 2 and res[5]["n_bases_left"] == 0
    res = run(hand_case(A60, B70, ["ACGTA", "ACGTA", "ACCTA", "TCGTA", "ACGTA"], backward=(0, 2)))
    assert M.strings(res) == [A60 + "ACGTA" + B70] and closure(res)["disputed"] == 2 and res[5]["disputed_cols"] == 2


def test_abutting_contigs():
    case = two_contigs(0, old_join=11)
    res = run(case)
    assert M.strings(res) == [case.text] and closure(res) == dict(status=M.ABUT, cands=3, reads=3, old=11, new=0, disputed=0, fill_pos=60)
    assert res[5]["abutted"] == 1 and res[5]["n_bases_left"] == 0


def overlap_case(A, B, o, flank=40):
    """reads that claim an overlap of o between A's right and B's left end: A's record stops one base short"""
    rows = []
    for i in range(2):
        rows += [rec(i, 0, max(len(A) - flank, 0), len(A) - 1, rstart=0, rstop=flank - 1, orient=i),
                 rec(i, 1, 0, min(len(B), flank), rstart=flank - o, rstop=flank - o + min(len(B), flank), orient=i)]
    members = np.array([(0, 0, 0, 0, (0, 0, 0)), (1, 6, 0, 0, (0, 0, 0))], dtype=SM.MEMBER_DTYPE)
    return CC.Case(None, [A, B], ["A" * 100] * 2, records(rows), CC.scaffold_records([2]), members)


def test_overlaps_verified_and_rejected():
    case = two_contigs(-20, old_join=6)
    res = run(case)
    assert M.strings(res) == [case.text] and closure(res) == dict(status=M.OVERLAP, cands=3, reads=3, old=6, new=-20, disputed=0, fill_pos=60)
    assert int(res[2][0]["overlap_bases"]) == 20 and res[5]["overlapped"] == 1
    spoiled = two_contigs(-20, old_join=6)
    spoiled.contigs[1] = spoiled.contigs[1][:7] + "N" + spoiled.contigs[1][8:]
    res = run(spoiled)
    assert closure(res) == dict(status=M.OVERLAP_REJECTED, cands=3, reads=3, old=6, new=6, disputed=0, fill_pos=60)
    assert M.strings(res) == [spoiled.contigs[0] + "N" * 6 + spoiled.contigs[1]] and res[5]["overlaps_rejected"] == 1
    # o = the shorter contig's length is no overlap, one less is
    A = A60
    res = run(overlap_case(A, A[-25:], 25))
    assert closure(res)["status"] == M.OVERLAP_REJECTED and M.strings(res) == [A + "N" * 6 + A[-25:]]
    res = run(overlap_case(A, A[-25:] + "G", 25))
    assert closure(res) == dict(status=M.OVERLAP, cands=2, reads=2, old=6, new=-25, disputed=0, fill_pos=60) and M.strings(res) == [A + "G"]
    res = run(overlap_case(A[-25:], "T" + A[-25:] + "G", 25))  # A is the shorter one
    assert closure(res)["status"] == M.OVERLAP_REJECTED


def test_joins_that_are_no_gaps_are_copied_and_their_reads_count_off_join():
    for g, old in ((7, 0), (7, -3), (0, 0)):
        case = two_contigs(g, old_join=old)
        res = run(case)
        t = case.contigs[0] + case.contigs[1][-old:]
        assert M.strings(res) == [t] and closure(res) == dict(status=M.NOT_A_GAP, cands=0, reads=0, old=old, new=old, disputed=0, fill_pos=60)
        assert res[5]["gaps"] == 0 and res[5]["cands"] == res[5]["cands_off_join"] == 3 and res[5]["passed"] == 6


def test_a_read_over_max_read_alns_and_candidates_off_the_join():
    case = hand_case(A60, B70, ["ACG", "ACG", "ACG"], extra_contigs=[CC.rand_seq(np.random.default_rng(9), 50)])
    extra = records([rec(0, 2, 10, 30, rstart=5, rstop=25)])
    case.alns = np.concatenate([case.alns, extra])
    res = run(case, max_read_alns=2)
    assert res[5]["reads_over_cap"] == 1 and closure(res)["cands"] == 2 and res[5]["cands"] == 2 and res[5]["passed"] == 7
    assert run(case, max_read_alns=3)[5]["reads_over_cap"] == 0
    # B -> A, and A -> the third contig, are candidates of no join of this scaffold; A -> B through the wrong strand neither
    rows = [rec(3, 1, 40, 70, rstart=0, rstop=30), rec(3, 0, 0, 30, rstart=33, rstop=63),
            rec(4, 0, 30, 60, rstart=0, rstop=30), rec(4, 2, 0, 30, rstart=32, rstop=62),
            rec(5, 0, 30, 60, rstart=0, rstop=30), rec(5, 1, 40, 70, rstart=0, rstop=30, orient=1)]
    case.alns = np.concatenate([case.alns[:6], records(rows)])
    case.reads += ["A" * 63] * 3
    res = run(case)
    assert res[5]["cands"] == 6 and res[5]["cands_off_join"] == 3 and closure(res)["cands"] == 3 and closure(res)["status"] == M.FILLED


def test_a_circular_scaffold_its_closing_join_has_no_member():
    case = hand_case(A60, B70, ["ACG", "ACG"])
    case.scaffolds = CC.scaffold_records([2], flags=[SM.CIRCULAR])
    rows = [rec(2, 1, 40, 70, rstart=0, rstop=30), rec(2, 0, 0, 30, rstart=33, rstop=63)]  # B -> A: the closing join
    case.alns = np.concatenate([case.alns, records(rows)])
    case.reads.append("C" * 63)
    res = run(case)
    assert M.strings(res) == [A60 + "ACG" + B70] and int(res[2][0]["flags"]) == SM.CIRCULAR and res[5]["cands_off_join"] == 1
    assert closure(res, 0)["status"] == M.HEAD and closure(res, 0)["cands"] == 0


# ---- invalid input ------------------------------------------------------------------------------------------------------------
def chain5():
    return CC.chain(5, seed=3)


def bad_scaffolds():
    yield "no member", lambda s, i: s.__setitem__(i, (int(s[i]["first_member"]), 0, 0, 0, 0, 0, (0, 0)))
    yield "not where its predecessor ends", lambda s, i: s.__setitem__(i, (int(s[i]["first_member"]) + 1, int(s[i]["n_members"]), 0, 0, 0, 0, (0, 0)))


def test_every_kind_of_invalid_scaffold_at_the_lowest_of_two():
    base = chain5()
    base.scaffolds = CC.scaffold_records([1, 1, 1, 1, 1])
    for m in range(5):
        base.members[m]["join"] = 0
    run(base)
    for name, spoil in bad_scaffolds():
        for idx in ((1,), (3,), (3, 1), (0,)):
            case = chain5()
            case.scaffolds, case.members = base.scaffolds.copy(), base.members.copy()
            for i in idx:
                spoil(case.scaffolds, i)
            with pytest.raises(M.BadScaffold) as e:
                M.close_gaps(*case.args())
            # a scaffold that starts one late makes its successor start early: the lowest of the two is named
            assert e.value.index == min(idx), (name, idx)
    for counts, bad in (([5, 1], 1), ([2, 2], 1), ([2, 4], 1), ([], 0), ([1, 1, 1, 1, 1, 1], 5)):
        case = chain5()
        case.scaffolds = CC.scaffold_records(counts)
        with pytest.raises(M.BadScaffold) as e:
            M.close_gaps(*case.args())
        assert e.value.index == bad, counts


def bad_members(case):
    """(name, spoil(members, i)) for i >= 1, a non-head of a scaffold of five"""
    other = lambda m, i: int(m[i - 1]["ctg"])
    yield "ctg out of range", lambda m, i: m[i].__setitem__("ctg", 5)
    yield "orient", lambda m, i: m[i].__setitem__("orient", 2)
    yield "reserved bytes", lambda m, i: m[i].__setitem__("pad", (0, 1, 0))
    yield "a contig twice", lambda m, i: m[i].__setitem__("ctg", other(m, i))
    yield "a join too long", lambda m, i: m[i].__setitem__("join", SM.INSERT_MAX + 1)
    yield "a join too short", lambda m, i: m[i].__setitem__("join", -SM.MAX_OVERLAP - 1)
    yield "an overlap as long as a contig", lambda m, i: m[i].__setitem__(
        "join", -min(len(case.contigs[int(m[i]["ctg"])]), len(case.contigs[int(m[i - 1]["ctg"])])))


def test_every_kind_of_invalid_member_at_the_lowest_of_two():
    for k in range(7):
        for idx in ((2,), (4,), (4, 2)):
            case = chain5()
            name, spoil = list(bad_members(case))[k]
            for i in idx:
                spoil(case.members, i)
            with pytest.raises(M.BadMember) as e:
                M.close_gaps(*case.args())
            assert e.value.index == min(idx), (name, idx)
    case = chain5()
    case.members[0]["join"] = 3  # a head's join
    with pytest.raises(M.BadMember) as e:
        M.close_gaps(*case.args())
    assert e.value.index == 0
    case = chain5()  # the longest overlap that is valid
    i = 2
    case.members[i]["join"] = 1 - min(len(case.contigs[int(case.members[i]["ctg"])]), len(case.contigs[int(case.members[i - 1]["ctg"])]))
    M.close_gaps(*case.args())
    case.members[i]["join"] = SM.INSERT_MAX
    M.close_gaps(*case.args())


def test_the_order_of_the_checks():
    case = chain5()
    case.members[3]["orient"] = 2
    case.scaffolds = CC.scaffold_records([2, 2])
    case.alns[4]["ctg"] = 9
    case.reads[1] = "A" * 1025
    with pytest.raises(D.BadRead):
        M.close_gaps(*case.args())
    case.reads[1] = "A" * 1024
    with pytest.raises(D.BadRecord) as e:
        M.close_gaps(*case.args())
    assert e.value.index == 4
    case.alns[4]["ctg"] = 0
    with pytest.raises(M.BadScaffold):
        M.close_gaps(*case.args())
    case.scaffolds = CC.scaffold_records([5])
    with pytest.raises(M.BadMember):
        M.close_gaps(*case.args())


BAD_PARAMS = [(dict(end_slack=1025), "kc_close_gaps: end_slack 1025 over 1024"),
              (dict(max_overlap=65536), "kc_close_gaps: max_overlap 65536 over 65535 or max_splint_gap 100 over 1024"),
              (dict(max_splint_gap=1025), "kc_close_gaps: max_overlap 200 over 65535 or max_splint_gap 1025 over 1024"),
              (dict(min_reads=0), "kc_close_gaps: min_reads 0 below 1"),
              (dict(min_agree_permille=1001), "kc_close_gaps: min_agree_permille 1001 over 1000"),
              (dict(max_read_alns=1), "kc_close_gaps: max_read_alns 1 outside 2 .. 64"),
              (dict(max_read_alns=65), "kc_close_gaps: max_read_alns 65 outside 2 .. 64"),
              (dict(flags=1), "kc_close_gaps: unknown flags 0x1")]
GOOD_PARAMS = [dict(end_slack=1024, max_overlap=65535, max_splint_gap=1024), dict(min_reads=1, min_agree_permille=1000), dict(max_read_alns=2),
               dict(max_read_alns=64, min_agree_permille=0, min_reads=0xFFFFFFFF)]


def test_every_parameter_error():
    case = two_contigs(7)
    for kw, text in BAD_PARAMS:
        with pytest.raises(D.BadArg) as e:
            M.close_gaps(*case.args(), **kw)
        assert str(e.value) == text
    for kw in GOOD_PARAMS:
        run(case, **kw)


def test_no_records_and_empty_contigs():
    case = CC.chain(4, seed=2)
    case.alns = case.alns[:0]
    res = run(case)
    want = "".join(("N" * int(m["join"])) + SM.node_text(case.contigs, 2 * int(m["ctg"]) + int(m["orient"])) for m in case.members)
    assert M.strings(res) == [want] and res[5]["gaps_no_reads"] == res[5]["gaps"] == 3 and res[5]["passed"] == 0
    assert [int(c["status"]) for c in res[4]] == [M.HEAD] + [M.NO_READS] * 3
    case.reads = []
    assert M.close_gaps(*case.args())[0] == res[0]
    # empty contigs: as a scaffold of their own, as a head and behind a gap
    members = np.array([(0, 0, 0, 0, (0, 0, 0)), (1, 0, 0, 1, (0, 0, 0)), (2, 2, 0, 0, (0, 0, 0))], dtype=SM.MEMBER_DTYPE)
    case = CC.Case(None, ["ACG", "", "T"], [], records([]), CC.scaffold_records([1, 2]), members)
    res = run(case)
    assert res[0] == b"ACG_NNT_" and list(res[1]) == [0, 4, 8] and [int(c["fill_pos"]) for c in res[4]] == [0, 4, 4]
    res = M.close_gaps([], [], records([]), CC.scaffold_records([]), members[:0])
    assert res[0] == b"" and list(res[1]) == [0]


# ---- the construction of tests/links_cases.py ---------------------------------------------------------------------------------
LINK_KW = dict(end_slack=0, max_overlap=50, max_splint_gap=50)


def layout_case(name):
    """the genome, and the construction's contigs, reads and records with the scaffolds scaffold_model makes of their links"""
    G, contigs, links = TS.layout_links(name)
    reads, places = LC.pairs_of(G, 19)
    alns = LC.geometric_records(LC.LAYOUTS[name][0], places)
    scaf = SM.scaffold(contigs, links.view(SM.LINK_DTYPE))
    return G, links, CC.Case(G, contigs, reads, alns, scaf[2], scaf[3])


@pytest.mark.parametrize("name", sorted(LC.LAYOUTS))
def test_the_end_to_end_construction_closes_to_the_genome(name):
    G, links, case = layout_case(name)
    res = run(case, **LINK_KW)
    assert M.strings(res) == [G[0:3000]] and res[5]["n_bases_left"] == 0 and len(res[2]) == 1
    by_ends = {(int(x["from"]), int(x["to"])): int(x["splints"]) for x in links}
    gap_joins = 0
    for m in range(1, 3):
        if int(case.members[m]["join"]) <= 0:
            assert closure(res, m)["status"] == M.NOT_A_GAP
            continue
        gap_joins += 1
        ea = (2 * int(case.members[m - 1]["ctg"]) + int(case.members[m - 1]["orient"])) ^ 1
        fb = 2 * int(case.members[m]["ctg"]) + int(case.members[m]["orient"])
        assert closure(res, m)["cands"] == by_ends[(ea, fb)] == closure(res, m)["reads"] and closure(res, m)["disputed"] == 0
    assert gap_joins == (2 if name == "gaps" else 1)
    if name == "gaps":  # checked once by hand: 9 splints over the 10-base gap, 4 over the 5-base gap, either direction among them
        assert [closure(res, m)["cands"] for m in (1, 2)] == [9, 4]
    # one base substituted inside the gap in the lowest-numbered supporter of each gap: outvoted, and counted
    st = dict.fromkeys(M.CLOSE_STATS, 0)
    cands = M.splints([len(c) for c in case.contigs], [len(r) for r in case.reads], case.alns, M.params(**LINK_KW), st)
    first = {}
    for r, X, Y, gap, s0, s1 in cands:
        if gap > 0:
            first.setdefault(frozenset((X, Y)), (r, s0))
    assert len(first) == gap_joins
    for r, s0 in first.values():
        t = case.reads[r]
        case.reads[r] = t[:s0] + "ACGT"[("ACGT".index(t[s0]) + 1) % 4] + t[s0 + 1:]
    res = run(case, **LINK_KW)
    assert M.strings(res) == [G[0:3000]]
    assert [closure(res, m)["disputed"] for m in range(1, 3) if closure(res, m)["status"] == M.FILLED] == [1] * gap_joins
    directions = {m: set() for m in (1, 2)}
    for r, X, Y, gap, s0, s1 in cands:
        for m in (1, 2):
            ea = (2 * int(case.members[m - 1]["ctg"]) + int(case.members[m - 1]["orient"])) ^ 1
            if gap > 0 and X in (ea, ) and int(case.members[m]["join"]) > 0:
                directions[m].add("forward")
            fb = 2 * int(case.members[m]["ctg"]) + int(case.members[m]["orient"])
            if gap > 0 and X == fb and Y == ea:
                directions[m].add("backward")
    assert all(d == {"forward", "backward"} for m, d in directions.items() if int(case.members[m]["join"]) > 0)
