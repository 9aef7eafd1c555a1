"""tests/dedup_model.py held to the rules of kc_ctg_dedup from outside: with max_mismatches = 0 it equals Python's `in` on
both strands for every anchored contig, every named container is kept, it is idempotent, a removal with mismatches is one a
brute-force search over every position finds too, and it gives the hand cases of tests/dedup_cases.py (no GPU needed)."""
import random

import numpy as np
import pytest

import dedup_cases as DC
import dedup_model as M


def random_block(r, k):
    """a few contigs cut from a small genome with N runs and a repeat; a third are contained, flipped or mutated copies"""
    g = bytearray(r.choice(b"ACGT") for _ in range(r.randrange(60, 400)))
    rep = g[10:10 + 3 * k]
    at = r.randrange(len(g))
    g[at:at] = rep
    for _ in range(r.randrange(3)):
        p = r.randrange(len(g))
        g[p:p + r.randrange(1, 2 * k)] = b"N" * r.randrange(1, 2 * k)
    ctgs = []
    for _ in range(r.randrange(2, 12)):
        p, n = r.randrange(len(g)), r.choice((0, k - 1, k, k + 1, 2 * k, 5 * k, 9 * k))
        ctgs.append(bytes(g[p:p + n]))
    for _ in range(len(ctgs) // 2):
        t = r.choice(ctgs)
        if len(t) > k:
            p = r.randrange(len(t) - k)
            t = t[p:p + r.randrange(k, len(t) - p + 1)]
        if r.random() < 0.5:
            t = M.rc(t)
        if t and r.random() < 0.3:
            t = bytearray(t)
            t[r.randrange(len(t))] = r.choice(b"ACGTN")
            t = bytes(t)
        ctgs.append(t)
    r.shuffle(ctgs)
    return ctgs


BLOCKS = [(seed, k, random_block(random.Random(seed), k)) for seed, k in ((s, (4, 5, 7, 8, 11)[s % 5]) for s in range(300))]


def test_exact_dedup_is_substring_containment_and_names_a_kept_container():
    removed = 0
    for seed, k, ctgs in BLOCKS:
        out = M.dedup(ctgs, k)
        recs = out["records"]
        for u, t in enumerate(ctgs):
            if recs["flags"][u] & M.UNANCHORED:
                assert recs["status"][u] == M.KEPT, (seed, u)
                continue
            inside = any(v != u and M.outranks(ctgs, v, u) and (t in tv or M.rc(t) in tv) for v, tv in enumerate(ctgs))
            assert (recs["status"][u] != M.KEPT) == inside, (seed, k, u, ctgs)
            if inside:
                removed += 1
                v = int(recs["container"][u])
                assert recs["status"][v] == M.KEPT and recs["mismatches"][u] == 0, (seed, u, v)
                j, side = int(recs["pos"][u]), M.rc(t) if recs["orient"][u] else t
                assert ctgs[v][j:j + len(t)] == side
                assert recs["status"][u] == (M.DUPLICATE if len(ctgs[v]) == len(t) else M.CONTAINED)
        assert out["ctgs"] == [t for u, t in enumerate(ctgs) if recs["status"][u] == M.KEPT]
        assert [int(x) for x in recs["absorbed"]] == [int(np.count_nonzero(recs["container"] == u)) for u in range(len(ctgs))]
    assert removed > 300  # the blocks do hold copies


def test_the_model_is_idempotent():
    for seed, k, ctgs in BLOCKS:
        for kw in (dict(), dict(duplicates_only=True)):
            once = M.dedup(ctgs, k, **kw)
            again = M.dedup(once["ctgs"], k, **kw)
            assert again["ctgs"] == once["ctgs"] and again["stats"]["kept"] == len(once["ctgs"]), (seed, kw)
            assert bytes(again["seqs"]) == bytes(once["seqs"]) and (again["offsets"] == once["offsets"]).all()


def test_a_removal_with_mismatches_is_one_brute_force_finds():
    for seed, k, ctgs in BLOCKS[:120]:
        for mm in (1, 2):
            recs = M.dedup(ctgs, k, max_mismatches=mm)["records"]
            for u in range(len(ctgs)):
                if recs["status"][u] != M.KEPT:
                    assert M.brute(ctgs, u, mm) and recs["mismatches"][u] <= mm, (seed, k, mm, u)
                    v, j = int(recs["container"][u]), int(recs["pos"][u])
                    assert M.mismatches(ctgs[u], ctgs[v], j, int(recs["orient"][u])) == recs["mismatches"][u]


def test_statistics_add_up_and_depths_follow_the_block():
    for seed, k, ctgs in BLOCKS[:60]:
        depths = [np.full(len(t), 7 + u, dtype=np.uint16) for u, t in enumerate(ctgs)]
        out = M.dedup(ctgs, k, depths=depths)
        st = out["stats"]
        assert st["kept"] + st["duplicates"] + st["contained"] == st["contigs"] == len(ctgs)
        assert st["kept_bases"] + st["removed_bases"] == st["bases"] and st["anchored"] + st["unanchored"] == len(ctgs)
        assert st["verified"] <= st["candidates"] and st["window_hits"] <= st["windows"]
        assert len(out["depths"]) == len(out["seqs"]) == st["kept_bases"] + st["kept"]
        for i, u in enumerate(out["kept"]):
            lo = int(out["offsets"][i])
            assert (out["depths"][lo:lo + len(ctgs[u])] == 7 + u).all() and out["depths"][lo + len(ctgs[u])] == 0


@pytest.mark.parametrize("k", DC.KS)
def test_hand_cases(k):
    for name, ctgs, kw, want in DC.cases(k):
        recs = M.dedup(ctgs, k, **kw)["records"]
        got = {u: (int(r["status"]), int(r["container"]), int(r["pos"]), int(r["orient"]), int(r["mismatches"]))
               for u, r in enumerate(recs) if r["status"] != M.KEPT}
        assert got == want, (k, name)


def test_the_candidate_limit_is_an_error_not_a_truncation():
    ctgs = [b"A" * (40 + i) for i in range(5)]  # poly-A contigs: every window of a longer one in which a shorter one fits
    st = M.dedup(ctgs, 21)["stats"]
    # a contig d bases longer holds the shorter one at d + 1 positions
    assert st["candidates"] == sum(d + 1 for u in range(5) for d in range(1, 5 - u)) == 30 and st["kept"] == 1
    with pytest.raises(M.Capacity, match="%d candidates, max_candidates is %d" % (st["candidates"], st["candidates"] - 1)):
        M.dedup(ctgs, 21, max_candidates=st["candidates"] - 1)
