"""tests/scaffold_model.py, the definition of kc_scaffold, on cases whose answer follows from the
case alone (no GPU needed).  tests/test_gpu_scaffold.py runs the same cases through the device, with this file's builders."""
import numpy as np
import pytest

import depth_model as D
import links_cases as LC
import links_model as LM
import scaffold_model as M
from scaffold_model import link, records, revc


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def texts(contigs, links, **kw):
    return M.strings(M.scaffold(contigs, links, **kw))


def members_of(res):
    return [(int(m["ctg"]), "+-"[int(m["orient"])], int(m["join"])) for m in res[3]]


def check_shape(contigs, res):
    """what holds for every result: the records describe the block, every contig is a member exactly once"""
    seqs, offsets, scafs, members, ctg_member, st = res
    assert len(members) == len(contigs) and sorted(int(m["ctg"]) for m in members) == list(range(len(contigs)))
    assert all(int(members[int(ctg_member[u])]["ctg"]) == u for u in range(len(contigs)))
    assert len(offsets) == len(scafs) + 1 and int(offsets[-1]) == len(seqs) and st["scaffolds"] == len(scafs)
    assert st["bases"] == len(seqs) - len(scafs) and st["longest"] == max([int(s["len"]) for s in scafs], default=0)
    assert st["edges_chosen"] == st["edges_joined"] + st["overlaps_rejected"]
    text = seqs.decode()
    heads = []
    for i, s in enumerate(scafs):
        a, b = int(offsets[i]), int(offsets[i + 1])
        assert text[b - 1] == "_" and b - 1 - a == int(s["len"])
        ms = members[int(s["first_member"]):int(s["first_member"]) + int(s["n_members"])]
        assert int(ms[0]["join"]) == 0
        heads.append(int(ms[0]["ctg"]))
        assert sum(max(int(m["join"]), 0) for m in ms) == int(s["n_bases"])
        assert sum(max(-int(m["join"]), 0) for m in ms) == int(s["overlap_bases"])
        for m in ms:
            t = contigs[int(m["ctg"])]
            t = revc(t) if int(m["orient"]) else t
            t = t[max(-int(m["join"]), 0):]
            assert text[int(m["out_pos"]):int(m["out_pos"]) + len(t)] == t
            assert text[int(m["out_pos"]) - max(int(m["join"]), 0):int(m["out_pos"])] == "N" * max(int(m["join"]), 0)
    assert heads == sorted(heads)


# ---- two contigs -------------------------------------------------------------------------------------------------------
def two_contigs(oa, ob, gap, rng=None):
    """contigs 0 and 1 such that node (0, oa) is followed by node (1, ob) at this gap: (contigs, links, the joined text)"""
    rng = rng or np.random.default_rng(5)
    A, B = rand_seq(rng, 60), rand_seq(rng, 45)
    if gap < 0:
        B = A[gap:] + B[-gap:]
    contigs = [revc(A) if oa else A, revc(B) if ob else B]
    e, f = (0 if oa else 1), (3 if ob else 2)  # (0, +) is left through end 1, (1, +) is entered through end 2
    text = A + "N" * max(gap, 0) + B[max(-gap, 0):]
    return contigs, records([link(e, f, splints=3, gap=gap)]), text


@pytest.mark.parametrize("gap", [7, 0, -20])
@pytest.mark.parametrize("oa,ob", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_two_contigs_in_all_four_orientation_pairs(oa, ob, gap):
    contigs, links, text = two_contigs(oa, ob, gap)
    res = M.scaffold(contigs, links)
    check_shape(contigs, res)
    assert M.strings(res) == [text]
    assert members_of(res) == [(0, "+-"[oa], 0), (1, "+-"[ob], gap)]
    assert res[5]["edges_joined"] == 1 and res[5]["overlaps_checked"] == (gap < 0) and res[5]["n_bases"] == max(gap, 0)
    assert res[5]["overlap_bases"] == max(-gap, 0) and res[5]["singletons"] == 0 and res[5]["scaffolds"] == 1


def test_the_twin_path_is_emitted_when_its_head_is_the_smaller_contig():
    # (1, +) -> (0, +): the emitted path starts at contig 0, so it is (0, -) -> (1, -)
    rng = np.random.default_rng(6)
    c = [rand_seq(rng, 30), rand_seq(rng, 50)]
    res = M.scaffold(c, records([link(3, 0, splints=2, gap=4)]))
    assert M.strings(res) == [revc(c[1] + "NNNN" + c[0])] and members_of(res) == [(0, "-", 0), (1, "-", 4)]
    check_shape(c, res)


# ---- a random graph: reverse complements and shuffles ---------------------------------------------------------------------
def random_case(seed, n=40, n_links=60):
    rng = np.random.default_rng(seed)
    contigs = [rand_seq(rng, int(rng.integers(1, 41))) for _ in range(n)]
    rows, seen = [], set()
    for _ in range(n_links):
        e, f = (int(x) for x in rng.integers(0, 2 * n, size=2))
        if e >> 1 == f >> 1 or (e, f) in seen or (f, e) in seen:
            continue
        seen.add((e, f))
        rows.append(link(e, f, splints=int(rng.integers(0, 4)), spans=int(rng.integers(1, 5)), gap=int(rng.integers(-3, 12)),
                         span_gap=int(rng.integers(-3, 30))))
    return contigs, rows


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reverse_complements_and_shuffled_numbers(seed):
    contigs, rows = random_case(seed)
    res = M.scaffold(contigs, records(rows), overlap_slack=2, max_second_permille=500)
    check_shape(contigs, res)
    assert res[5]["edges_joined"] >= 2
    # every contig reverse-complemented: its two ends change places, the scaffolds are the same with orientations flipped
    rows_rc = [(r[0] ^ 1, r[1] ^ 1) + tuple(r[2:]) for r in rows]
    rc = M.scaffold([revc(c) for c in contigs], records(rows_rc), overlap_slack=2, max_second_permille=500)
    # ... but for a single contig, which is emitted as (u, +), and a cycle, which is cut in front of (u*, +): those are read
    # from the other strand
    assert rc[5] == res[5] and len(rc[2]) == len(res[2])
    for a, b, ta, tb in zip(res[2], rc[2], M.strings(res), M.strings(rc)):
        ma = res[3][int(a["first_member"]):int(a["first_member"]) + int(a["n_members"])]
        mb = rc[3][int(b["first_member"]):int(b["first_member"]) + int(b["n_members"])]
        if int(a["n_members"]) == 1:
            assert tb == revc(ta) and ma.tobytes() == mb.tobytes()
        elif int(a["flags"]) & M.CIRCULAR:
            assert int(b["flags"]) & M.CIRCULAR and sorted(int(m["ctg"]) for m in ma) == sorted(int(m["ctg"]) for m in mb)
        else:
            assert ta == tb and a.tobytes() == b.tobytes()
            assert [(m["ctg"], m["join"], m["out_pos"], m["orient"] ^ 1) for m in mb] == [(m["ctg"], m["join"], m["out_pos"], m["orient"]) for m in ma]
    # shuffled contig numbers: the same texts, up to the strand and the order of the scaffolds
    rng = np.random.default_rng(seed + 100)
    perm = [int(x) for x in rng.permutation(len(contigs))]  # old -> new
    shuffled = [None] * len(contigs)
    for old, new in enumerate(perm):
        shuffled[new] = contigs[old]
    rows_sh = [(2 * perm[r[0] >> 1] + (r[0] & 1), 2 * perm[r[1] >> 1] + (r[1] & 1)) + tuple(r[2:]) for r in rows]
    sh = M.scaffold(shuffled, records(rows_sh), overlap_slack=2, max_second_permille=500)
    check_shape(shuffled, sh)
    # the supports are random, so two links of an end may tie and the smaller `to` decide, which the shuffle changes: the
    # texts are compared where the same edges were joined (test_shuffled_numbers_on_a_graph_without_ties has no ties)
    assert sh[5]["qualifying"] == res[5]["qualifying"] and sh[5]["ends_best"] == res[5]["ends_best"]


def test_shuffled_numbers_on_a_graph_without_ties():
    rng = np.random.default_rng(9)
    contigs = [rand_seq(rng, 20 + i) for i in range(6)]
    rows = [link(1, 2, splints=2, gap=3), link(3, 5, spans=3, gap=0), link(4, 6, splints=1, gap=9), link(8, 11, splints=4, gap=1)]
    base = texts(contigs, records(rows))
    assert len(base) == 2
    for perm in ([5, 4, 3, 2, 1, 0], [2, 0, 1, 5, 3, 4]):
        shuffled = [None] * 6
        for old, new in enumerate(perm):
            shuffled[new] = contigs[old]
        rows_sh = [(2 * perm[r[0] >> 1] + (r[0] & 1), 2 * perm[r[1] >> 1] + (r[1] & 1)) + tuple(r[2:]) for r in rows]
        got = texts(shuffled, records(rows_sh))
        assert sorted(min(t, revc(t)) for t in got) == sorted(min(t, revc(t)) for t in base)


# ---- thresholds and the choice -------------------------------------------------------------------------------------------
CTG3 = ["ACGTACGTAC", "GGATCCATTG", "TTGACCAGTA", "CATCATGGAC"]


def joined(links, n=4, **kw):
    """the chosen and joined edges as (smaller end, larger end, join)"""
    res = M.scaffold(CTG3[:n], links, **kw)
    check_shape(CTG3[:n], res)
    out = set()
    for s in res[2]:
        ms = res[3][int(s["first_member"]):int(s["first_member"]) + int(s["n_members"])]
        for a, b in zip(ms[:-1], ms[1:]):
            e, f = (2 * int(a["ctg"]) + int(a["orient"])) ^ 1, 2 * int(b["ctg"]) + int(b["orient"])
            out.add((min(e, f), max(e, f), int(b["join"])))
    return out, res[5]


def test_support_thresholds_at_and_one_under():
    assert joined(records([link(1, 2, splints=2, gap=1)]), min_splints=2)[0] == {(1, 2, 1)}
    assert joined(records([link(1, 2, splints=2, gap=1)]), min_splints=3)[0] == set()
    assert joined(records([link(1, 2, spans=2, gap=1)]))[0] == {(1, 2, 1)}  # the default: two spans
    assert joined(records([link(1, 2, spans=1, gap=1)]))[0] == set()
    assert joined(records([link(1, 2, spans=1, gap=1)]), min_spans=1)[0] == {(1, 2, 1)}
    # either kind is enough, and the gap is the splints' where there are any
    got, st = joined(records([link(1, 2, splints=1, spans=1, gap=2, span_gap=30)]), min_splints=1, min_spans=5)
    assert got == {(1, 2, 2)} and st["qualifying"] == 2
    got, st = joined(records([link(1, 2, splints=1, spans=5, gap=2, span_gap=30)]), min_splints=2, min_spans=5)
    assert got == {(1, 2, 2)}
    assert joined(records([link(1, 2, splints=1, spans=4, gap=2, span_gap=30)]), min_splints=2, min_spans=5)[0] == set()


def test_the_gap_is_the_mean_rounded_half_up_by_floor_division():
    def one(sum_, c):
        r = np.array([(1, 2, c, 0, -40, 40, 0, 0, sum_, 0), (2, 1, c, 0, -40, 40, 0, 0, sum_, 0)], dtype=M.LINK_DTYPE)
        return M.gap_of(r[0])
    assert [one(5, 2), one(-5, 2), one(7, 3), one(-7, 3), one(-1, 2), one(1, 2), one(-3, 2)] == [3, -2, 2, -2, 0, 1, -1]


def test_best_link_ties_permille_and_mutuality():
    # end 1 has two qualifying links: the greater support wins, any second makes it ambiguous at permille 0
    two = [link(1, 2, splints=3, gap=1), link(1, 4, splints=1, gap=2)]
    got, st = joined(records(two))
    assert got == set() and st["ends_ambiguous"] == 1 and st["ends_best"] == 3 and st["ends_not_mutual"] == 1
    # second.support * 1000 > best.support * permille: 1000 > 3 * 333 is ambiguous, 1000 > 3 * 334 is not
    assert joined(records(two), max_second_permille=333)[0] == set()
    got, st = joined(records(two), max_second_permille=334)
    assert got == {(1, 2, 1)} and st["ends_ambiguous"] == 0 and st["ends_not_mutual"] == 1  # end 4's best is end 1, whose best is 2
    # equal support: more splints win; equal splints: the smaller `to`
    tie = [link(1, 2, splints=1, spans=2, gap=1), link(1, 4, splints=2, spans=1, gap=2)]
    assert joined(records(tie), max_second_permille=1000)[0] == {(1, 4, 2)}
    tie = [link(1, 4, splints=2, gap=1), link(1, 2, splints=2, gap=5)]
    assert joined(records(tie), max_second_permille=1000)[0] == {(1, 2, 5)}
    # a second that does not qualify is no second
    assert joined(records([link(1, 2, splints=3, gap=1), link(1, 4, spans=1, gap=2)]))[0] == {(1, 2, 1)}
    # a best that is not mutual: 1 -> 2, but 2's best is 5
    got, st = joined(records([link(1, 2, splints=2, gap=1), link(2, 5, splints=5, gap=2)]), max_second_permille=1000)
    assert got == {(2, 5, 2)} and st["ends_not_mutual"] == 1 and st["edges_chosen"] == 1


def hub_case(partners, winner=None):
    """end 1 of contig 0 linked to the left ends of `partners` contigs; winner: the partner with ten times the support"""
    rng = np.random.default_rng(11)
    contigs = [rand_seq(rng, 12) for _ in range(partners + 1)]
    rows = [link(1, 2 * u, splints=20 if u == winner else 2, gap=u % 7) for u in range(1, partners + 1)]
    return contigs, records(rows)


def test_a_hub():
    contigs, links = hub_case(30)
    res = M.scaffold(contigs, links, max_second_permille=500)
    assert res[5]["scaffolds"] == 31 and res[5]["ends_ambiguous"] == 1 and res[5]["ends_not_mutual"] == 29
    contigs, links = hub_case(30, winner=17)
    res = M.scaffold(contigs, links, max_second_permille=500)
    assert res[5]["scaffolds"] == 30 and members_of(res)[:2] == [(0, "+", 0), (17, "+", 17 % 7)]
    check_shape(contigs, res)


# ---- the overlap search --------------------------------------------------------------------------------------------------
def overlap_case(true_o, claimed, la=40, lb=30, spoil=None, n_at=None, seed=3):
    """A then B sharing exactly true_o bytes (and no other overlap length nearby), the link claiming `claimed`"""
    rng = np.random.default_rng(seed)
    A = "A" * (la - true_o) + rand_seq(rng, true_o) if true_o < la else rand_seq(rng, la)
    A = "AC" * ((la - true_o) // 2) + "A" * ((la - true_o) % 2) + A[la - true_o:]
    B = A[la - true_o:] + ("GT" * lb)[:lb - true_o]
    if spoil is not None:  # a mismatch at this byte of the overlap, on B's side
        B = B[:spoil] + ("C" if B[spoil] != "C" else "G") + B[spoil + 1:]
    if n_at is not None:  # the same N on both sides
        A = A[:la - true_o + n_at] + "N" + A[la - true_o + n_at + 1:]
        B = B[:n_at] + "N" + B[n_at + 1:]
    return [A, B], records([link(1, 2, splints=2, gap=-claimed)])


def test_overlap_search():
    for claimed, slack, want in [(12, 0, -12), (13, 1, -12), (11, 1, -12), (17, 5, -12), (7, 5, -12), (18, 5, None), (6, 5, None), (13, 0, None)]:
        c, links = overlap_case(12, claimed)
        got = M.scaffold(c, links, overlap_slack=slack)
        assert (members_of(got)[1][2] if got[5]["edges_joined"] else None) == want, (claimed, slack)
        assert got[5]["overlaps_checked"] == 1 and got[5]["overlaps_rejected"] == (want is None)
        assert M.strings(got) == ([c[0] + c[1][12:]] if want else c)
        check_shape(c, got)
    for spoil in (0, 11):  # a mismatch at the overlap's first and last byte
        c, links = overlap_case(12, 12, spoil=spoil)
        assert M.scaffold(c, links)[5]["overlaps_rejected"] == 1
    c, links = overlap_case(12, 12, n_at=5)  # an N never matches, not even an N
    assert M.scaffold(c, links, overlap_slack=3)[5]["overlaps_rejected"] == 1
    # o' = min length - 1 is tried, min length itself is not
    c, links = overlap_case(29, 29, la=40, lb=30)
    assert members_of(M.scaffold(c, links))[1][2] == -29
    c = ["ACGTTGCAGGATC", "GTTGCAGGATC"]  # B is a suffix of A whole: o = |B| is refused, and no shorter overlap exists
    assert M.scaffold(c, records([link(1, 2, splints=2, gap=-11)]), overlap_slack=2)[5]["overlaps_rejected"] == 1
    # the nearer candidate wins, and o + d is tried before o - d
    c = ["GGGGGGAAAAAAAA", "AAAAAAAATTTTTT"]  # every overlap of 1 .. 8 verifies
    for claimed, want in [(5, -5), (9, -8), (12, None)]:
        got = M.scaffold(c, records([link(1, 2, splints=2, gap=-claimed)]), overlap_slack=3)
        assert (members_of(got)[1][2] if got[5]["edges_joined"] else None) == want
    c = ["GGGGGGACACACAC", "ACACACACTTTTTT"]  # overlaps of 2, 4, 6, 8 verify: claimed 5 finds 6 before 4
    assert members_of(M.scaffold(c, records([link(1, 2, splints=2, gap=-5)]), overlap_slack=3))[1][2] == -6


# ---- chains and cycles ---------------------------------------------------------------------------------------------------
def chain_of(lens, joins, strands, order, seed=1, cycle_join=None):
    """contigs cut from one text: position i of the chain is contig order[i] with lens[i] bases on strand strands[i], joined
    to its predecessor by joins[i] (negative: a true overlap of that many bases; joins[0] is not read); cycle_join closes
    the chain.  Returns (contigs, links)."""
    rng = np.random.default_rng(seed)
    contigs, rows, prev = [None] * len(lens), [], None
    for i, u in enumerate(order):
        t = rand_seq(rng, lens[i])
        if i and joins[i] < 0:
            o = -joins[i]
            assert 1 <= o < min(len(t), len(prev))
            t = prev[-o:] + t[o:]
        contigs[u] = revc(t) if strands[i] else t
        if i:
            e, f = 2 * order[i - 1] + (0 if strands[i - 1] else 1), 2 * u + (1 if strands[i] else 0)
            rows.append(link(e, f, splints=2, gap=joins[i]))
        prev = t
    if cycle_join is not None and len(lens) >= 2:
        e, f = 2 * order[-1] + (0 if strands[-1] else 1), 2 * order[0] + (1 if strands[0] else 0)
        rows.append(link(e, f, splints=2, gap=cycle_join))
    return contigs, records(rows)


def chain_case(n, seed=1, cycle=False, lens=(1, 41), gaps=(-3, 9)):
    """n contigs of random lengths, numbers and strands in a chain (or a cycle) with random true gaps and overlaps"""
    rng = np.random.default_rng(seed)
    order = [int(x) for x in rng.permutation(n)]
    strands = [int(x) for x in rng.integers(0, 2, size=n)]
    ls = [int(x) for x in rng.integers(lens[0], lens[1], size=n)]
    js = [int(x) for x in rng.integers(gaps[0], gaps[1], size=n)]
    for i in range(1, n):  # an overlap is shorter than either text
        if js[i] < 0:
            js[i] = -min(-js[i], ls[i] - 1, ls[i - 1] - 1)
    return chain_of(ls, js, strands, order, seed=seed + 1000, cycle_join=2 if cycle else None)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_chains(n):
    contigs, links = chain_case(n, seed=n)
    res = M.scaffold(contigs, links)
    check_shape(contigs, res)
    assert res[5]["scaffolds"] == 1 and res[5]["edges_joined"] == n - 1 and int(res[2][0]["n_members"]) == n and res[5]["circular"] == 0


def test_a_chain_whose_higher_numbered_end_heads_neither_emitted_path():
    # 2 - 0 - 1: the path from contig 2 and its twin from contig 1; the head is the smaller of the two, contig 1
    rng = np.random.default_rng(2)
    c = [rand_seq(rng, 10), rand_seq(rng, 12), rand_seq(rng, 14)]
    res = M.scaffold(c, records([link(5, 0, splints=2, gap=1), link(1, 2, splints=2, gap=2)]))
    assert members_of(res) == [(1, "-", 0), (0, "-", 2), (2, "-", 1)]
    assert M.strings(res) == [revc(c[2] + "N" + c[0] + "NN" + c[1])]


@pytest.mark.parametrize("n", [2, 3])
def test_cycles_with_the_smallest_contig_in_every_position(n):
    for seed in range(8):
        contigs, links = chain_case(n, seed=seed, cycle=True, gaps=(0, 5))
        res = M.scaffold(contigs, links)
        check_shape(contigs, res)
        assert res[5]["circular"] == 1 and res[5]["scaffolds"] == 1 and res[5]["edges_joined"] == n
        assert int(res[2][0]["flags"]) == M.CIRCULAR and members_of(res)[0] == (0, "+", 0) and int(res[2][0]["n_members"]) == n


# ---- invalid input -------------------------------------------------------------------------------------------------------
GOOD = records([link(1, 2, splints=2, spans=1, gap=-3, span_gap=4), link(3, 5, spans=2, gap=7), link(1, 6, splints=1, gap=0)])


def spoiled(i, **kw):
    x = GOOD.copy()
    for k, v in kw.items():
        x[i][k] = v
    return x


def invalid_cases():
    """(records, the lowest bad index): every kind of invalid record alone"""
    n = 2 * len(CTG3)
    yield spoiled(0, **{"from": n}), 0
    yield spoiled(1, to=n), 1
    yield spoiled(5, to=7), 1  # (6, 1) -> (6, 7), two ends of contig 3: its mirror, record 1, breaks first
    yield spoiled(2, to=3), 0  # (2, 1) -> (2, 3): record 0's mirror is gone
    yield records([link(0, 2, splints=1), link(2, 3, splints=1)]), 2  # (0, 2) (2, 0) (2, 3) (3, 2): two ends of contig 1, mirrored
    yield spoiled(3, splints=0, spans=0, span_gap_min=0, span_gap_max=0, span_gap_sum=0), 3  # no supporter
    yield spoiled(3, splint_gap_min=1), 3  # a kind with count 0 and a field
    yield spoiled(3, splint_gap_sum=1), 3
    yield spoiled(0, splint_gap_min=-65536, splint_gap_sum=-65536 - 3), 0
    yield spoiled(0, span_gap_max=65536, span_gap_sum=65536), 0
    yield spoiled(0, splint_gap_min=-2), 0  # min above max
    yield spoiled(0, splint_gap_sum=-7), 0  # below c * min
    yield spoiled(0, span_gap_sum=5), 0  # above c * max
    yield GOOD[[1, 0, 2, 3, 4, 5]], 1  # record 1 is not above its predecessor (the search still finds record 0's mirror)
    yield GOOD[[0, 0, 1, 2, 3, 4, 5]], 1  # a key twice
    yield GOOD[[0, 1, 3, 4, 5]], 0  # record 0's mirror is gone
    yield spoiled(2, spans=2, span_gap_min=4, span_gap_max=4, span_gap_sum=8), 0  # the mirror's figures differ
    yield spoiled(2, splint_gap_sum=-5, splint_gap_min=-3, splint_gap_max=-2), 0


def test_every_kind_of_invalid_record_alone_and_at_two_indices():
    assert M.first_invalid(GOOD, 4) is None and M.first_invalid(GOOD[:0], 4) is None
    for links, bad in invalid_cases():
        assert M.first_invalid(links, 4) == bad, (links, bad)
        with pytest.raises(M.BadArg, match="record %d is invalid" % bad):
            M.scaffold(CTG3, links)
    two = spoiled(4, splint_gap_min=9)
    two[1]["to"] = 99
    assert M.first_invalid(two, 4) == 1
    assert M.first_invalid(GOOD, 3) == 1  # ends 6 and 7 do not exist: record 1 is (1, 6)


BAD_PARAMS = [(dict(min_splints=0), "kc_scaffold: min_splints 0, min_spans 2 below 1"), (dict(min_spans=0), "kc_scaffold: min_splints 1, min_spans 0 below 1"),
              (dict(max_second_permille=1001), "kc_scaffold: max_second_permille 1001 over 1000"),
              (dict(overlap_slack=65), "kc_scaffold: overlap_slack 65 over 64"), (dict(flags=1), "kc_scaffold: unknown flags 0x1")]


def test_every_parameter_error():
    for kw, text in BAD_PARAMS:
        with pytest.raises(M.BadArg) as e:
            M.scaffold(CTG3, GOOD, **kw)
        assert str(e.value) == text
    for kw in (dict(min_splints=1, min_spans=1), dict(max_second_permille=1000), dict(overlap_slack=64), dict(min_splints=0xFFFFFFFF)):
        M.scaffold(CTG3, GOOD, **kw)


def test_no_links_and_empty_contigs():
    res = M.scaffold(["ACG", "", "T"], records([]))
    assert res[0] == b"ACG__T_" and list(res[1]) == [0, 4, 5, 7] and res[5]["singletons"] == 3
    res = M.scaffold(["ACG", "", "T"], records([link(1, 2, splints=1, gap=2), link(3, 4, splints=1, gap=-1)]), overlap_slack=4)
    assert res[0] == b"ACGNN_T_" and members_of(res) == [(0, "+", 0), (1, "+", 2), (2, "+", 0)] and res[5]["overlaps_rejected"] == 1
    check_shape(["ACG", "", "T"], res)


# ---- the construction of tests/links_cases.py ---------------------------------------------------------------------------------
def layout_links(name):
    layout, gaps = LC.LAYOUTS[name]
    G = LC.genome(19)
    reads, places = LC.pairs_of(G, 19)
    alns = LC.geometric_records(layout, places)
    ctg_lens, read_lens = [b - a for a, b, _ in layout], [len(r) for r in reads]
    _, pairs, _ = D.pair_inserts(ctg_lens, read_lens, alns, 1000)
    links, _, _ = LM.ctg_links(ctg_lens, read_lens, alns, pairs, insert_avg=LC.FRAGMENT, max_insert=1000, end_slack=0, max_overlap=50, max_splint_gap=50)
    return G, LC.contigs_of(G, layout), links


def layout_text(name, G):
    if name == "gaps":
        return G[0:1000] + 10 * "N" + G[1010:2000] + 5 * "N" + G[2005:3000]
    return G[0:2000] + 5 * "N" + G[2005:3000]


@pytest.mark.parametrize("name", sorted(LC.LAYOUTS))
def test_the_end_to_end_construction_gives_the_genome_back(name):
    G, contigs, links = layout_links(name)
    res = M.scaffold(contigs, links.view(M.LINK_DTYPE))
    check_shape(contigs, res)
    assert M.strings(res) == [layout_text(name, G)]
    assert members_of(res) == [(0, "+", 0), (1, "+", 10 if name == "gaps" else -20), (2, "-", 5)]
    assert res[5]["scaffolds"] == 1 and res[5]["edges_joined"] == 2 and res[5]["overlaps_checked"] == (name == "overlap")
