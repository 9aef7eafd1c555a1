"""The host model of the read-to-contig alignment (tests/align_model.py) against properties that hold by construction,
on random contigs and reads at k = 5, 6, 21, 32, 33.  No GPU, no library."""
import numpy as np
import pytest

import align_model as M

KS = (5, 6, 21, 32, 33)


def rand_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def unique_contigs(rng, k, n_ctgs=4, length=400):
    """Random contigs in which every k-mer is a seed (drawn again until that holds: at k = 5 and 6 the contigs are short)."""
    length = min(length, {5: 14, 6: 24}.get(k, length))
    for _ in range(2000):
        ctgs = [rand_seq(rng, length + 3 * u) for u in range(n_ctgs)]
        ix = M.Index(*M.join_block(ctgs), k)
        if ix.stats["repeated"] == 0:
            return ctgs, ix
    raise AssertionError("no repeat-free contigs found")


@pytest.mark.parametrize("k", KS)
def test_read_cut_from_a_contig(k):
    rng = np.random.default_rng(100 + k)
    ctgs, ix = unique_contigs(rng, k)
    for u, ctg in enumerate(ctgs):
        for L in (k, k + 1, min(len(ctg), 3 * k)):
            a = int(rng.integers(0, len(ctg) - L + 1))
            read = ctg[a:a + L]
            for s in (1, 3):
                starts = len(range(0, L - k + 1, s))
                recs, (windows, hits, rep, perfect) = M.align_read(ix, read, s, 0)
                assert recs == [(u, a, a + L, 0, L, 0, starts, 0)]
                assert (windows, hits, rep, perfect) == (starts, starts, 0, 1)
                # the reverse-complemented read: the same contig interval, orient 1
                recs, _ = M.align_read(ix, M.revcomp(read), s, 0)
                assert recs == [(u, a, a + L, 0, L, 0, starts, 1)]


@pytest.mark.parametrize("k", KS)
def test_one_substitution_loses_the_windows_that_cover_it(k):
    rng = np.random.default_rng(200 + k)
    ctgs, ix = unique_contigs(rng, k)
    ctg = ctgs[1]
    L = min(len(ctg), 3 * k + 2)
    a = int(rng.integers(0, len(ctg) - L + 1))
    for x in (0, k - 1, L // 2, L - 1):
        read = list(ctg[a:a + L])
        read[x] = "ACGT"[("ACGT".index(read[x]) + 1) % 4]
        read = "".join(read)
        covering = sum(1 for p in range(L - k + 1) if p <= x < p + k)
        recs, _ = M.align_read(ix, read, 1, M.KEEP_ALL)
        mine = [r for r in recs if r[0] == 1 and r[7] == 0 and r[1] - r[3] == a]
        # (a window with the substituted base may by chance be another seed: that is another candidate, not this one)
        assert mine == [(1, a, a + L, 0, L, 1, L - k + 1 - covering, 0)]
        assert M.align_read(ix, read, 1, 0)[0] == [r for r in recs if r[5] == 0]


@pytest.mark.parametrize("k", KS)
def test_records_are_unique_and_sorted(k):
    rng = np.random.default_rng(300 + k)
    ctgs, ix = unique_contigs(rng, k)
    reads = []
    for _ in range(40):
        u, v = rng.integers(0, len(ctgs), size=2)
        a = ctgs[u][int(rng.integers(0, len(ctgs[u]) - k)):][:2 * k]
        b = ctgs[v][int(rng.integers(0, len(ctgs[v]) - k)):][:2 * k]
        read = a + b
        reads.append(M.revcomp(read) if rng.integers(0, 2) else read)
    alns, first, st = M.align_reads(ix, reads)
    assert alns.dtype.itemsize == 32 and len(first) == len(reads) + 1 and first[-1] == len(alns) == st["alignments"]
    keys = [(int(a["read"]), int(a["ctg"]), int(a["orient"]), int(a["cstart"]) - int(a["rstart"])) for a in alns]
    assert keys == sorted(set(keys))
    for r in range(len(reads)):
        assert all(int(a["read"]) == r for a in alns[int(first[r]):int(first[r + 1])])
    assert st["reads_aligned"] == len(reads) and not alns["pad"].any()


@pytest.mark.parametrize("k", KS)
def test_a_kmer_in_two_contigs_is_no_seed(k):
    rng = np.random.default_rng(400 + k)
    ctgs, ix = unique_contigs(rng, k)
    shared = ctgs[0][3:3 + k]
    ctgs2 = ctgs + [rand_seq(rng, 4) + M.revcomp(shared) + rand_seq(rng, 4)]  # the other strand counts as the same k-mer
    ix2 = M.Index(*M.join_block(ctgs2), k)
    rc = M.revcomp(shared)
    key = rc if rc < shared else shared
    assert ix.seeds[key] is not None and ix2.seeds[key] is None
    assert ix2.stats["repeated"] >= 1 and ix2.stats["windows"] > ix.stats["windows"]
    recs, (windows, hits, rep, _) = M.align_read(ix2, shared, 1, M.KEEP_ALL)
    assert recs == [] and (windows, hits, rep) == (1, 0, 1)


def test_palindromes_ns_and_block_checks():
    pal = "ACGT" * 2  # its own reverse complement (even k only)
    ix = M.Index(*M.join_block(["TT" + pal + "GG", "", "ACNGTACCA"]), 8)
    assert ix.seeds[pal] is None and ix.stats["contigs"] == 3 and ix.stats["bases"] == 21
    assert ix.stats["windows"] == 5 + 0 + 0  # no window covers the N: ACNGTACC, CNGTACCA
    assert M.check_block("ACGT_", [0, 5]) is None
    assert M.check_block("ACxT_", [0, 5]) == "KC_ERR_BAD_BASE"
    assert M.check_block("acgt_", [0, 5]) == "KC_ERR_BAD_BASE"
    assert M.check_block("ACGT_AC_", [0, 4, 8]) == "KC_ERR_INVALID_ARG"
    assert M.check_block("ACGT_AC_", [0, 5]) == "KC_ERR_INVALID_ARG"
    assert M.check_block("ACGT_AC", [0, 5, 7]) == "KC_ERR_INVALID_ARG"
    assert M.check_block("", [0]) is None
