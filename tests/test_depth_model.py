"""tests/depth_model.py against cases whose answer follows from the case alone (no GPU needed)."""
import numpy as np
import pytest

import depth_model as D
from depth_model import rec, records


def depths_of(out, ctg_lens, u):
    o = D.block_offsets(ctg_lens)
    return [int(x) for x in out[o[u]:o[u] + ctg_lens[u]]]


def test_one_record():
    lens = [10, 0, 4]
    out, ctgs, st = D.aln_depths(lens, records([rec(0, 0, 2, 5)]))
    assert len(out) == 10 + 1 + 0 + 1 + 4 + 1
    assert [int(x) for x in out] == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert ctgs[0].tolist() == (3, 10, 3, 0, 1, 1, 0)  # mean floor((3 + 5) / 10) = 0
    assert ctgs[1].tolist() == (0, 0, 0, 0, 0, 0, 0) and ctgs[2].tolist() == (0, 4, 0, 0, 0, 0, 0)
    assert st == dict(records=1, none=0, filtered=0, not_best=0, clipped_away=0, used=1, bases_covered=3, depth_sum=3, saturated=0)


def test_records_tiling_a_contig():
    lens = [3, 12]
    alns = records([rec(i, 1, 4 * i, 4 * i + 4) for i in range(3)] + [rec(9, 1, 0, 12)])
    out, ctgs, st = D.aln_depths(lens, alns)
    assert depths_of(out, lens, 1) == [2] * 12 and depths_of(out, lens, 0) == [0] * 3
    assert ctgs[1].tolist() == (24, 12, 12, 2, 2, 4, 2)
    assert st["used"] == 4 and st["bases_covered"] == 12 and st["depth_sum"] == 24


def test_edge_clip_at_a_start_an_end_and_inside():
    lens = [20]
    at_start, at_end, inside = rec(0, 0, 0, 8), rec(1, 0, 12, 20), rec(2, 0, 5, 15)
    out, _, _ = D.aln_depths(lens, records([at_start]), edge_clip=3)
    assert depths_of(out, lens, 0) == [1] * 5 + [0] * 15  # the contig's own start is kept, the other end loses 3
    out, _, _ = D.aln_depths(lens, records([at_end]), edge_clip=3)
    assert depths_of(out, lens, 0) == [0] * 15 + [1] * 5
    out, _, _ = D.aln_depths(lens, records([inside]), edge_clip=3)
    assert depths_of(out, lens, 0) == [0] * 8 + [1] * 4 + [0] * 8
    out, _, _ = D.aln_depths(lens, records([rec(0, 0, 0, 20)]), edge_clip=1024)
    assert depths_of(out, lens, 0) == [1] * 20  # both ends are the contig's
    out, _, _ = D.aln_depths(lens, records([rec(0, 0, 1, 19)]), edge_clip=2)
    assert depths_of(out, lens, 0) == [0] * 3 + [1] * 14 + [0] * 3  # one off either end: clipped


def test_edge_clip_eating_the_whole_interval():
    lens = [20]
    for e, want in ((4, 2), (5, 0), (6, 0), (1024, 0)):
        out, ctgs, st = D.aln_depths(lens, records([rec(0, 0, 5, 15)]), edge_clip=e)
        assert sum(depths_of(out, lens, 0)) == want
        assert (st["clipped_away"], st["used"], int(ctgs[0]["alns"])) == ((0, 1, 1) if want else (1, 0, 0))
    with pytest.raises(D.BadArg):
        D.aln_depths(lens, records([]), edge_clip=1025)
    with pytest.raises(D.BadArg):
        D.aln_depths(lens, records([]), flags=4)


def test_filter_none_and_validity():
    lens = [30, 5]
    alns = records([rec(0, 0, 0, 10, score=20), rec(0, 0, 0, 10, score=19), rec(0, 0, 0, 9, score=50), (7, 1, 0, 0, 0, 0, 0, 0, 0, 0, D.KIND_NONE, (0, 0))])
    out, ctgs, st = D.aln_depths(lens, alns, min_score=20, min_len=10)
    assert (st["none"], st["filtered"], st["used"]) == (1, 2, 1) and depths_of(out, lens, 0)[:10] == [1] * 10
    for i, bad in enumerate([rec(0, 2, 0, 1), rec(0, 0, 0, 31), rec(0, 0, 5, 5), rec(0, 0, 0, 4, rstart=4, rstop=4), rec(0, 0, 0, 4, rstart=1021, rstop=1025),
                             rec(0, 0, 0, 4, orient=2), rec(0, 0, 0, 4, kind=3), (0, 2, 0, 0, 0, 0, 0, 0, 0, 0, D.KIND_NONE, (0, 0))]):
        with pytest.raises(D.BadRecord) as e:
            D.aln_depths(lens, np.concatenate([alns, records([bad]), alns, records([bad])]))
        assert e.value.index == 4, i
    # the read field is read only with BEST_ONLY
    D.aln_depths(lens, records([rec(99, 0, 0, 4)]))
    with pytest.raises(D.BadRecord):
        D.aln_depths(lens, records([rec(99, 0, 0, 4)]), flags=D.BEST_ONLY, nreads=99)
    D.aln_depths(lens, records([rec(98, 0, 0, 4)]), flags=D.BEST_ONLY, nreads=99)


def test_best_only_and_the_tie_on_equal_scores():
    lens = [40]
    alns = records([rec(0, 0, 0, 10, score=30), rec(0, 0, 10, 20, score=40), rec(0, 0, 20, 30, score=40), rec(1, 0, 30, 40, score=5),
                    rec(0, 0, 0, 40, score=99, kind=D.KIND_NONE)])
    assert D.best_records(alns, 2, 0, 0) == [1, 3]  # the greatest score, the lowest index; a NONE record never
    out, ctgs, st = D.aln_depths(lens, alns, flags=D.BEST_ONLY, nreads=2)
    assert depths_of(out, lens, 0) == [0] * 10 + [1] * 10 + [0] * 10 + [1] * 10
    assert (st["not_best"], st["used"], st["none"]) == (2, 2, 1)
    assert D.best_records(alns[[2, 1, 0, 3, 4]], 2, 0, 0) == [0, 3]  # the tie follows the array, not the record
    assert D.best_records(alns, 2, 41, 0) == [None, None] and D.best_records(alns, 2, 0, 11) == [None, None]


def test_mean_rounds_half_up_and_per_contig_fills():
    # depth_sum / len = 1.5 exactly -> 2; 1.25 -> 1; 2.5 -> 3 (len even: len / 2 is exact); len 3, sum 4: 4/3 -> 1; sum 5: 5/3 -> 2
    for n, cover, want in ((4, [4, 2], 2), (4, [4, 1], 1), (2, [2, 2, 1], 3), (3, [3, 1], 1), (3, [3, 2], 2)):
        lens = [2, n, 0, 1]
        out, ctgs, _ = D.aln_depths(lens, records([rec(i, 1, 0, c) for i, c in enumerate(cover)]), flags=D.PER_CONTIG)
        assert int(ctgs[1]["mean"]) == want and int(ctgs[1]["depth_sum"]) == sum(cover)
        assert [int(x) for x in out] == [0, 0, 0] + [want] * n + [0] + [0] + [0, 0]
    out, ctgs, st = D.aln_depths([2], records([rec(0, 0, 0, 2)] * 70000))
    assert ctgs[0].tolist() == (140000, 2, 2, 70000, 70000, 70000, 65535) and [int(x) for x in out] == [65535, 65535, 0]
    assert st["saturated"] == 2


def pair(f, r, read_lens=(100, 100), max_insert=500):
    alns = records([x for x in (f, r) if x is not None])
    return D.pair_inserts([1000, 1000], list(read_lens), alns, max_insert)


def test_every_pair_class():
    F = rec(0, 0, 100, 200, orient=0)
    hist, pairs, st = pair(F, rec(1, 0, 250, 350, orient=1))
    assert pairs[0].tolist()[:4] == (0, 1, 250, D.PAIR_PROPER) and int(hist[250]) == 1 and int(hist.sum()) == 1
    assert (st["insert_sum"], st["insert_sq_sum"], st["reads_with_best"], st["cls"]) == (250, 62500, 2, [0, 0, 0, 0, 0, 0, 1])
    assert pair(None, None)[1][0].tolist()[:4] == (D.NO_ALN, D.NO_ALN, 0, D.PAIR_NONE)
    assert pair(F, None)[1][0].tolist()[:4] == (0, D.NO_ALN, 0, D.PAIR_ONE)
    assert pair(None, rec(1, 0, 250, 350, orient=1))[1][0].tolist()[:4] == (D.NO_ALN, 0, 0, D.PAIR_ONE)
    assert pair(F, rec(1, 1, 250, 350, orient=1))[1][0].tolist()[:4] == (0, 1, 0, D.PAIR_DIFF_CTG)
    assert pair(F, rec(1, 0, 250, 350, orient=0))[1][0].tolist()[:4] == (0, 1, 0, D.PAIR_SAME_ORIENT)
    assert pair(rec(0, 0, 100, 200, orient=1), rec(1, 0, 250, 350, orient=1))[1][0].tolist()[:4] == (0, 1, 0, D.PAIR_SAME_ORIENT)
    assert pair(F, rec(1, 0, 99, 199, orient=1))[1][0].tolist()[:4] == (0, 1, 0, D.PAIR_EVERTED)
    assert pair(F, rec(1, 0, 100, 200, orient=1))[1][0].tolist()[:4] == (0, 1, 100, D.PAIR_PROPER)  # rs == fs: f = L
    assert pair(F, rec(1, 0, 500, 600, orient=1))[1][0].tolist()[:4] == (0, 1, 500, D.PAIR_PROPER)
    hist, pairs, st = pair(F, rec(1, 0, 501, 601, orient=1))
    assert pairs[0].tolist()[:4] == (0, 1, 501, D.PAIR_TOO_LONG) and int(hist.sum()) == 0 and st["insert_sum"] == 0
    # mate 1 the reverse one: the same fragment
    assert pair(rec(0, 0, 250, 350, orient=1), rec(1, 0, 100, 200, orient=0))[1][0].tolist()[:4] == (0, 1, 250, D.PAIR_PROPER)
    # soft clips are projected: F misses its first 7 bases, R (120 bases) the last 20 of R'
    got = pair(rec(0, 0, 107, 200, rstart=7, orient=0), rec(1, 0, 250, 350, rstart=0, rstop=100, orient=1), read_lens=(100, 120))
    assert got[1][0].tolist()[:4] == (0, 1, 370 - 100, D.PAIR_PROPER)
    # a mate over the contig's start: fs is negative
    got = pair(rec(0, 0, 0, 60, rstart=40, orient=0), rec(1, 0, 50, 150, orient=1))
    assert got[1][0].tolist()[:4] == (0, 1, 190, D.PAIR_PROPER)


def test_pair_arguments_and_validity():
    for bad in (0, 65536):
        with pytest.raises(D.BadArg):
            D.pair_inserts([10], [5, 5], records([]), bad)
    with pytest.raises(D.BadArg):
        D.pair_inserts([10], [5, 5, 5], records([]), 100)
    with pytest.raises(D.BadRead) as e:
        D.pair_inserts([10], [5, 1025], records([]), 100)
    assert e.value.index == 1
    ok = rec(1, 0, 0, 5)
    D.pair_inserts([10], [5, 5], records([ok]), 100)
    for bad in (rec(2, 0, 0, 5), rec(1, 0, 0, 6), rec(1, 0, 0, 5, rstart=1, rstop=6)):
        with pytest.raises(D.BadRecord) as e:
            D.pair_inserts([10], [5, 5], records([ok, bad]), 100)
        assert e.value.index == 1
    # a NONE record needs a read, but no interval
    D.pair_inserts([10], [5, 5], records([(1, 0, 0, 0, 0, 0, 0, 0, 0, 0, D.KIND_NONE, (0, 0))]), 100)
    with pytest.raises(D.BadRecord):
        D.pair_inserts([10], [5, 5], records([(2, 0, 0, 0, 0, 0, 0, 0, 0, 0, D.KIND_NONE, (0, 0))]), 100)
