"""tests/shuffle_model.py against cases whose answer follows from the case alone (no device): the choice of a pair's home
tie by tie, the order inside a segment, the dealing over the parts against a brute-force dealing, and the invariants of
a shuffle over tests/links_cases.py's genome."""
import numpy as np
import pytest

import links_cases as LC
import shuffle_model as M
from depth_model import NO_ALN, PAIR_DTYPE, rec, records

LENS = [300, 250, 400]


def build(specs, read_len=20, seed=0, lens=None):
    """specs: one (mate 0, mate 1) a pair, a mate None or (ctg, cstart, score): (bases, quals, offsets, alns, pairs) with a
    record for every mate that has one, reads of random text, lengths read_len or one list entry a read"""
    rng = np.random.default_rng(seed)
    nreads = 2 * len(specs)
    lens = [read_len] * nreads if lens is None else lens
    offsets = np.zeros(nreads + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    total = int(offsets[-1])
    bases = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=total).astype(np.uint8)
    quals = rng.integers(33, 74, size=total).astype(np.uint8)
    rows, pairs = [], np.zeros(len(specs), dtype=PAIR_DTYPE)
    for p, mates in enumerate(specs):
        for side, m in enumerate(mates):
            name = "aln%d" % side
            if m is None or lens[2 * p + side] == 0:
                pairs[p][name] = NO_ALN
                continue
            ctg, cstart, score = m
            n = min(10, lens[2 * p + side])
            pairs[p][name] = len(rows)
            rows.append(rec(2 * p + side, ctg, cstart, cstart + n, rstart=0, rstop=n, score=score))
    return bases, quals, offsets, records(rows) if rows else np.zeros(0, dtype=M.GAP_ALN_DTYPE), pairs


def run(specs, parts=1, ctg_lens=LENS, **kw):
    bases, quals, offsets, alns, pairs = build(specs, **kw)
    out = M.shuffle_reads(ctg_lens, bases.tobytes(), quals.tobytes(), offsets, alns, pairs, parts)
    out["order_"] = np.frombuffer(out["order"], dtype=np.uint32).tolist()
    out["home_"] = np.frombuffer(out["home"], dtype=np.uint32).tolist()
    out["starts_"] = np.frombuffer(out["part_starts"], dtype=np.uint64).tolist()
    return out


def test_the_choice_rule_tie_by_tie():
    # the greater score wins, whichever mate has it and whatever the contig
    assert run([((2, 50, 30), (0, 5, 31))])["home_"] == [0]
    assert run([((2, 50, 31), (0, 5, 30))])["home_"] == [2]
    # equal scores: the smaller contig
    assert run([((2, 50, 30), (1, 90, 30))])["home_"] == [1]
    assert run([((1, 90, 30), (2, 50, 30))])["home_"] == [1]
    # equal scores on one contig: the smaller cstart is the anchor -- seen in the order of two pairs around it
    out = run([((1, 90, 30), (1, 40, 30)), ((1, 60, 30), None)])
    assert out["order_"] == [0, 1] and out["home_"] == [1, 1]
    out = run([((1, 90, 30), (1, 70, 30)), ((1, 60, 30), None)])
    assert out["order_"] == [1, 0]
    out = run([((1, 40, 30), (1, 90, 30)), ((1, 60, 30), None)])
    assert out["order_"] == [0, 1]
    # all equal: mate 0, which changes nothing but is the record the rule names
    a = records([rec(0, 1, 40, 50, score=30), rec(1, 1, 40, 50, score=30)])
    assert M.choose(a[0], a[1]) is not None and int(M.choose(a[0], a[1])["read"]) == 0
    assert int(M.choose(None, a[1])["read"]) == 1 and M.choose(None, None) is None


def test_one_mate_only_and_the_statistics():
    out = run([(None, (2, 7, 5)), ((0, 9, 5), None), (None, None), ((1, 3, 9), (1, 8, 2)), ((1, 3, 2), (0, 8, 9))])
    assert out["order_"] == [4, 1, 3, 0, 2] and out["home_"] == [0, 0, 1, 2, M.NO_HOME]
    st = out["stats"]
    assert (st["pairs"], st["homed"], st["homeless"], st["one_mate"], st["two_same"], st["two_diff"]) == (5, 4, 1, 2, 1, 1)
    assert (st["homes"], st["max_home_pairs"], st["bytes"]) == (3, 2, 200)
    assert st["key_bits"] == (400).bit_length() + (3).bit_length() == 11


def test_all_homeless_and_all_on_one_contig():
    out = run([(None, None)] * 5, parts=2)
    assert out["order_"] == [0, 1, 2, 3, 4] and out["home_"] == [M.NO_HOME] * 5 and out["starts_"] == [0, 2, 5]
    assert (out["stats"]["homes"], out["stats"]["max_home_pairs"], out["stats"]["homeless"]) == (0, 0, 5)
    out = run([((1, c, 30), None) for c in (50, 10, 30, 10, 0)])
    assert out["order_"] == [4, 1, 3, 2, 0] and out["home_"] == [1] * 5
    assert (out["stats"]["homes"], out["stats"]["max_home_pairs"]) == (1, 5)


def test_equal_keys_keep_the_old_order():
    specs = [((1, 10, 30), None), (None, None), ((1, 10, 99), (2, 0, 1)), ((0, 10, 30), None), ((1, 10, 30), (1, 10, 30)), (None, None)]
    out = run(specs)
    assert out["order_"] == [3, 0, 2, 4, 1, 5]


def brute_force_parts(n, parts):
    """the part of every rank of a segment of n pairs, by the statement of the rule"""
    return [next(j for j in range(parts) if j * n // parts <= r < (j + 1) * n // parts) for r in range(n)]


@pytest.mark.parametrize("nh,nu", [(0, 9), (9, 0), (5, 4), (1, 1), (13, 3)])
def test_the_parts_against_a_brute_force_dealing(nh, nu):
    specs = [((p % 3, 5 * p, 30), None) for p in range(nh)] + [(None, None)] * nu
    rng = np.random.default_rng(nh * 16 + nu)
    specs = [specs[i] for i in rng.permutation(len(specs))]
    n = nh + nu
    flat = run(specs, parts=1)
    homed, homeless = flat["order_"][:nh], flat["order_"][nh:]
    assert flat["home_"][nh:] == [M.NO_HOME] * nu and M.NO_HOME not in flat["home_"][:nh] and flat["starts_"] == [0, n]
    for parts in (1, 2, 7, n + 3):
        out = run(specs, parts=parts)
        ph, pu = brute_force_parts(nh, parts), brute_force_parts(nu, parts)
        want = []
        for j in range(parts):
            want += [homed[r] for r in range(nh) if ph[r] == j] + [homeless[r] for r in range(nu) if pu[r] == j]
        assert out["order_"] == want
        assert out["starts_"] == [sum(1 for x in ph if x < j) + sum(1 for x in pu if x < j) for j in range(parts + 1)]
        assert out["starts_"][parts] == n
        # the closed form of a rank's part
        assert ph == [((r + 1) * parts - 1) // nh for r in range(nh)] and pu == [((r + 1) * parts - 1) // nu for r in range(nu)]
        sizes = np.diff(out["starts_"])
        assert sizes.max() - sizes.min() <= 2  # each segment is dealt to within one pair


def test_the_bytes_move_with_their_pair():
    lens = [0, 1, 15, 16, 17, 150, 1024, 3, 0, 0, 16, 16]
    specs = [((2, 9, 3), None), (None, (1, 4, 3)), (None, None), ((0, 7, 3), (0, 1, 3)), (None, None), ((2, 2, 1), None)]
    bases, quals, offsets, alns, pairs = build(specs, lens=lens)
    out = M.shuffle_reads(LENS, bases.tobytes(), quals.tobytes(), offsets, alns, pairs, 2)
    order = np.frombuffer(out["order"], dtype=np.uint32).tolist()
    # pair 0's only candidate would be a read of length 0, which has no record: homed are (0, 1) pair 3, (1, 4) pair 1 and
    # (2, 2) pair 5, homeless pairs 0, 2, 4; part 0 takes one of each, part 1 two of each
    assert order == [3, 0, 1, 5, 2, 4]
    noff = np.frombuffer(out["offsets"], dtype=np.uint64).tolist()
    for q, p in enumerate(order):
        for s in (0, 1):
            a, b = int(offsets[2 * p + s]), int(offsets[2 * p + s + 1])
            assert out["bases"][noff[2 * q + s]:noff[2 * q + s + 1]] == bases.tobytes()[a:b]
            assert out["quals"][noff[2 * q + s]:noff[2 * q + s + 1]] == quals.tobytes()[a:b]
    assert noff[-1] == int(offsets[-1]) == len(out["bases"])
    got = np.frombuffer(out["gap_alns"], dtype=M.GAP_ALN_DTYPE)
    new_of = {p: q for q, p in enumerate(order)}
    assert [int(x) for x in got["read"]] == [2 * new_of[int(r) >> 1] + (int(r) & 1) for r in alns["read"]]
    assert np.frombuffer(out["pairs"], dtype=PAIR_DTYPE).tobytes() == pairs[order].tobytes()
    no_q = M.shuffle_reads(LENS, bases.tobytes(), None, offsets, alns, pairs, 2)
    assert no_q["quals"] is None and no_q["bases"] == out["bases"]


def test_what_is_refused():
    bases, quals, offsets, alns, pairs = build([((1, 10, 30), (2, 0, 1)), (None, None)])
    args = (LENS, bases.tobytes(), None)
    for parts in (0, M.MAX_PARTS + 1):
        with pytest.raises(M.BadArg):
            M.shuffle_reads(*args, offsets, alns, pairs, parts)
    with pytest.raises(M.BadArg):
        M.shuffle_reads(*args, offsets[:-1], alns, pairs)
    long_offsets = offsets.copy()
    long_offsets[3:] += 1100
    with pytest.raises(M.BadRead) as e:
        M.shuffle_reads(*args, long_offsets, alns, pairs)
    assert e.value.index == 2
    back = offsets.copy()
    back[2] = 10
    with pytest.raises(M.BadRead) as e:
        M.shuffle_reads(*args, back, alns, pairs)
    assert e.value.index == 1
    bad = alns.copy()
    bad[1]["ctg"] = 3
    with pytest.raises(M.BadRecord) as e:
        M.shuffle_reads(*args, offsets, bad, pairs)
    assert e.value.index == 1
    q = pairs.copy()
    q[1]["aln0"] = 0  # a record of another read
    with pytest.raises(M.BadPair) as e:
        M.shuffle_reads(*args, offsets, alns, q)
    assert e.value.index == 1
    out = M.shuffle_reads(LENS, b"", None, np.zeros(1, dtype=np.uint64), alns[:0], pairs[:0], 3)
    assert out["offsets"] == bytes(8) and out["part_starts"] == bytes(32) and out["stats"]["key_bits"] == 0


def dealt_case(seed=19, name="gaps"):
    """tests/links_cases.py's genome and pairs, the pairs dealt in random order, with the records their geometry gives"""
    layout, _ = LC.LAYOUTS[name]
    G = LC.genome(seed)
    reads, places = LC.pairs_of(G, seed)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(reads) // 2)
    reads = [reads[2 * p + s] for p in perm for s in (0, 1)]
    places = [places[2 * p + s] for p in perm for s in (0, 1)]
    ctg_lens = [b - a for a, b, _ in layout]
    return ctg_lens, reads, LC.geometric_records(layout, places)


def test_invariants_on_the_links_genome():
    ctg_lens, reads, alns = dealt_case()
    read_lens = [len(r) for r in reads]
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.asarray(read_lens, dtype=np.uint64))
    bases = "".join(reads).encode()
    _, pairs, _ = M.pair_inserts(ctg_lens, read_lens, alns)
    npairs = len(pairs)
    for parts in (1, 3):
        out = M.shuffle_reads(ctg_lens, bases, None, offsets, alns, pairs, parts)
        order = np.frombuffer(out["order"], dtype=np.uint32).tolist()
        home = np.frombuffer(out["home"], dtype=np.uint32).tolist()
        starts = np.frombuffer(out["part_starts"], dtype=np.uint64).tolist()
        noff = np.frombuffer(out["offsets"], dtype=np.uint64).tolist()
        assert sorted(order) == list(range(npairs))
        text = out["bases"].decode()
        assert [text[noff[i]:noff[i + 1]] for i in range(len(reads))] == [reads[2 * p + s] for p in order for s in (0, 1)]
        new_alns = np.frombuffer(out["gap_alns"], dtype=M.GAP_ALN_DTYPE)
        new_pairs = np.frombuffer(out["pairs"], dtype=PAIR_DTYPE)
        # the shuffled reads with the renumbered records classify as the old ones did
        _, again, _ = M.pair_inserts(ctg_lens, [read_lens[2 * p + s] for p in order for s in (0, 1)], new_alns)
        assert again.tobytes() == new_pairs.tobytes()
        st = out["stats"]
        assert st["homed"] + st["homeless"] == npairs and st["homed"] == st["one_mate"] + st["two_same"] + st["two_diff"] > 0
        assert st["homes"] == len(ctg_lens) and st["two_diff"] > 0
        for j in range(parts):
            h = [x for x in home[starts[j]:starts[j + 1]]]
            nh = sum(1 for x in h if x != M.NO_HOME)
            assert all(x != M.NO_HOME for x in h[:nh]) and all(x == M.NO_HOME for x in h[nh:])
            assert h[:nh] == sorted(h[:nh])
            anchors = []
            for q in range(starts[j], starts[j] + nh):
                c = [new_alns[int(new_pairs[q][n])] for n in ("aln0", "aln1") if int(new_pairs[q][n]) != NO_ALN]
                b = M.choose(c[0], c[1]) if len(c) == 2 else c[0]
                assert int(b["ctg"]) == home[q]
                anchors.append((home[q], int(b["cstart"])))
            assert anchors == sorted(anchors)
