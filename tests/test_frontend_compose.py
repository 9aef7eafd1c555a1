"""CPU checks of what the exact GPU comparisons of the front end (tests/test_gpu_frontend_scale.py and the edge tests of
the merge and trim modules) are built from: the per-item results and compose() of tests/merge_model.py and
tests/trim_model.py against the models themselves, the row-block prefilter against the whole-window one, and that every
seeded family holds what it is for, counted from the models alone."""
import json
import os

import numpy as np

import merge_model as M
import trim_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "merge_hand_cases.json")))["cases"]
FA_PATH = os.path.join(HERE, "golden", "adapters_no_transposase.fa")
FA = open(FA_PATH, "rb").read()
FA_SEQS = T.read_fasta_seqs(FA_PATH)


def _prefilter_inputs(pair, qoff=33):
    s1 = np.frombuffer(pair[0].encode() if isinstance(pair[0], str) else pair[0], dtype=np.uint8)
    s2 = np.frombuffer(pair[2].encode() if isinstance(pair[2], str) else pair[2], dtype=np.uint8)
    ln = min(len(s1), len(s2))
    return s1, len(s1) - ln, M.COMP[s2[::-1]], ln, ln - M.MIN_OVERLAP + M.EXTRA_TEST_OVERLAP


def test_prefilter_in_row_blocks_is_the_whole_window():
    pairs = [c["pair"] for c in CASES] + M.random_pairs(np.random.default_rng(11), 2000)
    ran = 0
    for pr in pairs:
        s1, start, rc, ln, ntr = _prefilter_inputs(pr)
        if ntr <= 0:
            continue
        want = M._prefilter_counts_whole(s1, start, rc, ln, ntr)
        for block in (1, 1000, 1 << 22):  # one row a block, a few rows, everything at once
            got = M.prefilter_counts(s1, start, rc, ln, ntr, block)
            assert got.dtype == want.dtype and np.array_equal(got, want)
        ran += 1
    assert ran > 1800


def test_merge_compose_identity_and_shuffle():
    rng = np.random.default_rng(71)
    pairs = M.random_pairs(rng, 2500) + [c["pair"] for c in CASES if c["qual_offset"] == 33] + M.cross_chunk_pairs(n=300)
    items = M.MergeItems(pairs)
    b, q, o = M.interleave(pairs)
    want = M.merge_pairs(b, q, o)
    got = items.compose(np.arange(len(pairs)))
    assert np.array_equal(got[0], b) and np.array_equal(got[1], q) and np.array_equal(got[2], o)
    assert np.array_equal(got[3], want[0]) and np.array_equal(got[4], want[1]) and got[5] == want[2]
    assert got[4].dtype == want[1].dtype and got[2].dtype == o.dtype
    order = rng.integers(0, len(pairs), 4000)  # repeats and omissions
    cb, cq, co, cp, coo, cst = items.compose(order)
    wb, wq, wo = M.interleave([pairs[i] for i in order])
    assert np.array_equal(cb, wb) and np.array_equal(cq, wq) and np.array_equal(co, wo)
    dp, do, dst = M.merge_pairs(cb, cq, co)
    assert np.array_equal(cp, dp) and np.array_equal(coo, do) and cst == dst
    assert cst["merged"] > 500 and cst["dropped"] > 20 and cst["ambiguous"] > 50
    # an empty arrangement, and small gather chunks
    eb, eq, eo, ep, eoo, est = items.compose([])
    assert len(eb) == 0 and eo.tolist() == [0] and eoo.tolist() == [0] and est["pairs"] == 0 and est["out_reads"] == 0
    st, ln = items.in_start[order], (items.len1 + items.len2)[order]
    assert np.array_equal(M.gather_segments(items.bases, st, ln, chunk=7), cb)


def test_merge_pair_ex_reports_the_stop():
    by = {c["name"]: c for c in CASES}

    def info(name):
        c = by[name]
        b, q, o = M.interleave([c["pair"]])
        a, e, z = int(o[0]), int(o[1]), int(o[2])
        r = M.merge_pair_ex(b[a:e], q[a:e], b[e:z], q[e:z], c["qual_offset"], c["min_kmer_len"])
        assert (r[0], r[1]) == M.merge_pair(b[a:e], q[a:e], b[e:z], q[e:z], c["qual_offset"], c["min_kmer_len"])
        return r[2]
    i = info("clean_overlap")
    assert i["rule"] == "end" and i["best"] == 20 and i["stop"] == i["ntr"] - 1 and (20, "good") in i["events"]
    assert info("two_good_offsets")["rule"] == "good_after_best"
    assert info("good_after_found")["rule"] == "good_after_weak"
    assert info("both_ns_twice")["rule"] == "abort_both_ns"
    assert info("ncount_over_3")["rule"] == "abort_ncount"
    assert info("both_short_dropped") == dict(ntr=0, stop=-1, rule="dropped", best=-1, events=[])
    for n in ("two_good_offsets", "good_after_found", "both_ns_twice", "ncount_over_3"):
        assert info(n)["best"] == -1 and info(n)["stop"] == info(n)["events"][-1][0]


def test_length_grid_holds_every_residue_and_chunk_edge():
    pairs = M.length_grid_pairs()
    items = M.MergeItems(pairs)
    assert len(pairs) > 4000
    merged = items.stats[:, 0] == 1
    best = np.array([i["best"] for i in items.info])
    ln = np.minimum(items.len1, items.len2)
    start = items.len1 - ln
    # all four residues of the funnel shift and of the loops' ends, together, at the static and the dynamic path
    for long in (False, True):
        sel = merged & (items.is_long() == long)
        seen = set(zip(((start + best)[sel] & 3).tolist(), ((ln - best)[sel] & 3).tolist()))
        assert len(seen) == 16, (long, seen)
    # every pair of lengths occurs, and each that leaves room merges at every chunk edge
    for l1 in M.GRID_LENS:
        for l2 in M.GRID_LENS:
            sel = (items.len1 == l1) & (items.len2 == l2)
            assert sel.any()
            fit = {i for i in M.GRID_OFFSETS if min(l1, l2) - i >= M.MIN_OVERLAP and max(l1, l2) >= 21}  # else dropped
            assert fit <= set(best[sel & merged].tolist()), (l1, l2)
            assert (sel & ~merged).any()
    # 74 and 138 bases give 64 and 128 trials; the last one with an overlap of 12 is offset 62 and 126
    assert set(best[merged & (ln == 74)].tolist()) >= {62} and set(best[merged & (ln == 75)].tolist()) >= {62, 63}
    assert set(best[merged & (ln == 139)].tolist()) >= {127} and set(best[merged & (ln >= 255)].tolist()) >= {128, 129}
    assert (items.stats[:, 2] == 1).sum() >= 9 and (~merged & (items.stats[:, 2] == 0)).sum() > 600


def test_cross_chunk_family_decides_in_later_chunks():
    """Counted from the model's stop report.  The fourth kind the family was asked for, an abort at an offset of 64 or
    more after a good trial below 64, cannot exist under the reference's rules: a good trial has checked its whole
    overlap with Ncount <= 3 (or aborts itself and ends the loop), a later trial compares a sub-range of both mates
    (mate 1 from start + i on, the reversed mate 2 up to len - i), so it meets no more Ns than the earlier one, and both
    aborts need four (two matched pairs, or Ncount > 3).  Aborts at 64 and beyond are there without it."""
    items = M.MergeItems(M.cross_chunk_pairs())
    count = {}
    for inf in items.info:
        for k in M.classify_cross_chunk(inf):
            count[k] = count.get(k, 0) + 1
    print(count, "merged", int(items.stats[:, 0].sum()), "of", len(items))
    for k in ("merged_late", "best_then_later_chunk", "weak_then_later_good", "weak_only_in_earlier_chunks", "abort_late"):
        assert count.get(k, 0) >= 200, (k, count)
    assert count.get("abort_late_after_early_good", 0) == 0
    assert items.stats[:, 0].sum() * 5 >= len(items)
    assert items.len1.min() >= 150 and items.len1.max() <= 500
    stops = np.array([i["stop"] for i in items.info if i["rule"] != "end"])
    assert (stops >= 128).sum() > 100 and (stops >= 192).sum() > 30  # third and fourth chunk too


def test_long_path_family_is_what_it_says():
    pairs = M.long_path_pairs()
    items = M.MergeItems(pairs)
    assert items.is_long().all()
    key = {(int(a), int(b)): n for n, (a, b) in enumerate(zip(items.len1, items.len2))}
    assert items.info[key[(32767, 32767)]]["best"] == 0 and items.stats[key[(32767, 32767)], 3] == 32767
    assert items.stats[key[(32767, 13)], 0] == 1 and items.stats[key[(13, 32767)], 0] == 1
    assert items.stats[key[(20000, 600)], 0] == 1 and items.stats[key[(600, 20000)], 0] == 1
    assert max(i["best"] for i in items.info) > 10000
    for ln in range(513, 521):
        assert ((items.len1 == ln) | (items.len2 == ln)).sum() >= 3
    has_n = np.array([b"N" in p[0] for p in pairs])
    assert (has_n & (items.stats[:, 0] == 1)).sum() >= 2 and (has_n & (items.stats[:, 1] >= 1)).sum() >= 2
    assert (items.stats[:, 0] == 0).sum() >= 4
    # with min_kmer_len above them, the pairs just over the static buffers are dropped
    d = M.MergeItems([p for p in pairs if max(len(p[0]), len(p[2])) <= 520], min_len=600)
    assert len(d) >= 20 and d.stats[:, 2].all()


def test_trim_compose_identity_and_shuffle():
    b, q, o = T.random_pairs(8, 1500, FA_SEQS)
    ads = T.AdapterSet(FA, 21)
    items = T.TrimItems(ads, b, q, o)
    rng = np.random.default_rng(72)
    for paired in (True, False):
        n = 1500 if paired else 3000
        want = T.trim_reads(ads, b, q, o, paired, list(items.per_read))
        got = items.compose(np.arange(n), paired)
        assert np.array_equal(got[0], b) and np.array_equal(got[1], q) and np.array_equal(got[2], o)
        assert all(np.array_equal(x, y) for x, y in zip(got[3:6], want[:3])) and got[6] == want[3]
        assert got[5].dtype == want[2].dtype
        order = rng.integers(0, n, 1000 if paired else 2000)
        cb, cq, co, wb, wq, wo, wst = items.compose(order, paired)
        db, dq, do, dst = T.trim_reads(ads, cb, cq, co, paired)  # the model on the composed input, from scratch
        assert np.array_equal(wb, db) and np.array_equal(wq, dq) and np.array_equal(wo, do) and wst == dst
        assert wst["trimmed"] > 200 and wst["alignments"] >= wst["trimmed"]


def test_seed_position_family_is_found_only_on_the_stride():
    for k in (29, 32):
        ads = T.AdapterSet(FA, k)
        ad = [s for s in FA_SEQS if len(s) >= 60][0]
        fam = T.seed_position_reads(ads, ad)
        b, q, o = T.reads_to_arrays([r for r, _, _ in fam])
        res = T.trim_per_read(ads, b, o)
        on = {p for (_, p, hit) in fam if hit}
        assert {0, 4, 216, 220, 224, 228, 444, 448} <= on
        assert {len(r) for r, _, _ in fam} >= {k - 1, k, k + 1, 223 + k, 224 + k, 225 + k, 448 + k}
        for (r, pos, hit), (ln, trimmed, nal) in zip(fam, res):
            assert nal == (1 if hit else 0), (k, len(r), pos)  # a neighbour of the stride is never aligned
            if not hit:
                assert (ln, trimmed) == (len(r), False)
        assert sum(1 for _, p, hit in fam if not hit and p >= 0) > 40
