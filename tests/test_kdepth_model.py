"""tests/kdepth_model.py, the model the device tests of kc_seq_kmer_depths and kc_count_spectrum compare with, held three
ways that do not go through it: against a dictionary of packed k-mers cut by the oracle's get_kmers, against a genome whose
track is known by construction, and by the symmetry of the two strands.  No GPU needed."""
import numpy as np
import pytest

import kdepth_model as M
from helpers import random_reads
from oracle import cpu_oracle as O

KS = (21, 31, 32, 33, 63, 64, 65, 99)


def oracle_table(reads, quals, k):
    (keys, counts, _, _), _ = O.count_reads(reads, quals, k=k)
    return keys, counts


@pytest.mark.parametrize("k", KS)
def test_model_equals_a_dictionary_of_packed_kmers(k):
    rng = np.random.default_rng(k)
    reads, quals = random_reads(rng, 300, min_len=max(3, k - 3), max_len=k + 60, genome_len=700, err=0.01)
    keys, counts = oracle_table(reads, quals, k)
    assert len(counts) > 100
    brute = {tuple(int(w) for w in key): int(c) for key, c in zip(keys, counts)}
    tab = M.table(keys, counts, k)
    # sequences without a non-base, which is all get_kmers cuts: a few reads and pieces of the genome the results came from
    seqs = [r for r in reads[:40] if set(r) <= set("ACGT")] + ["", "A" * (k - 1), "ACGT" * k]
    assert len(seqs) > 10
    sb, offs = M.block(seqs)
    track, recs, stats = M.kmer_depths(tab, k, sb, offs, min_count=3)
    for i, s in enumerate(seqs):
        want = []
        for w in O.get_kmers(s, k):
            rc = O.revcomp(w, k)
            want.append(brute.get(min(tuple(int(x) for x in w), tuple(int(x) for x in rc)), 0))
        a = int(offs[i])
        assert list(track[a:a + len(want)]) == want and not track[a + len(want):int(offs[i + 1])].any()
        present = [c for c in want if c]
        assert (recs[i]["sum"], recs[i]["windows"], recs[i]["present"], recs[i]["solid"]) == (sum(want), len(want), len(present), sum(c >= 3 for c in want))
        assert (recs[i]["min_count"], recs[i]["max_count"]) == ((min(present), max(present)) if present else (0, 0))
        assert recs[i]["mean"] == (int(sum(want) / len(want) + 0.5) if want else 0)
    assert stats["present"] > 100 and stats["longest"] == max(len(s) for s in seqs) and stats["seqs"] == len(seqs)
    assert stats["sum"] == int(recs["sum"].sum()) and stats["bytes"] == len(sb)


@pytest.mark.parametrize("m", (2, 3, 255))
@pytest.mark.parametrize("k", (21, 33, 64))
def test_identical_reads_of_a_repeat_free_genome(k, m):
    g = M.unique_genome(np.random.default_rng(7 * k + m), 400, k)
    reads = [g.decode()] * m
    keys, counts = oracle_table(reads, None, k)
    sb, offs = M.block([g])
    track, recs, stats = M.kmer_depths(M.table(keys, counts, k), k, sb, offs)
    # the first and the last k-mer have no neighbour on one side, a dead end, and are purged
    want = np.zeros(len(g), dtype=np.uint16)
    want[1:len(g) - k] = m
    assert (track == want).all()
    assert recs[0]["windows"] == len(g) - k + 1 and recs[0]["present"] == recs[0]["solid"] == len(g) - k - 1 and recs[0]["sum"] == m * (len(g) - k - 1)
    hist, st = M.spectrum(counts)
    assert hist[m] == len(g) - k - 1 and hist.sum() == hist[m]
    assert st == dict(kmers=len(g) - k - 1, sum_counts=m * (len(g) - k - 1), max_count=m, mode_count=m, mode_kmers=len(g) - k - 1, saturated=0)
    assert M.format_spectrum(hist) == "%d %d\n" % (m, len(g) - k - 1)
    filled = M.kmer_depths(M.table(keys, counts, k), k, sb, offs, fill_mean=True)[0]
    assert (filled == M.mean_of(m * (len(g) - k - 1), len(g) - k + 1)).all()


@pytest.mark.parametrize("k", (21, 32, 77))
def test_the_other_strand_has_the_track_reversed(k):
    rng = np.random.default_rng(5 + k)
    reads, quals = random_reads(rng, 300, min_len=k, max_len=k + 80, genome_len=600, err=0.01)
    tab = M.table(*oracle_table(reads, quals, k), k)
    seqs = [r.encode() for r in reads[:30]] + [b"ACGTNNacgt" * 12, b"_", (reads[0][:k + 5] + "_" + reads[1]).encode()]
    for s in seqs:
        fwd = M.kmer_depths(tab, k, *M.block([s]))
        rev = M.kmer_depths(tab, k, *M.block([M.revcomp(s.translate(bytes.maketrans(b"acgt", b"ACGT")))]))
        nwin = max(len(s) - k + 1, 0)
        assert (fwd[0][:nwin] == rev[0][:nwin][::-1]).all() and not fwd[0][nwin:].any()
        for name in M.REC_DTYPE.names[:-1]:
            assert fwd[1][name] == rev[1][name], name
        assert fwd[2] == rev[2]


def test_non_bases_case_sequence_ends_and_nothing():
    k = 5
    tab = {b"AACCG": 7, b"ACCGG": 2}
    assert M.canonical(b"CCGGT") == b"ACCGG" and M.canonical(b"ccGgt") == b"ACCGG"  # one key for both strands, and for lower case
    sb, offs = M.block(["AACCGGT", "aaccggt", "AACCNGGT", "AACC", "", "GGT_AACCG", b"AACC\xffAACCG", "AACCG"])
    track, recs, stats = M.kmer_depths(tab, k, sb, offs, min_count=7)
    assert list(track[:7]) == [7, 2, 2, 0, 0, 0, 0] and list(track[7:14]) == list(track[:7])
    assert not track[14:22].any() and not track[22:26].any()  # an N in every window; too short
    assert list(track[26:35]) == [0, 0, 0, 0, 7, 0, 0, 0, 0]  # no window across the '_' or the sequence's end
    assert list(track[35:45]) == [0] * 5 + [7] + [0] * 4 and list(track[45:]) == [7, 0, 0, 0, 0]
    assert [int(x) for x in recs["windows"]] == [3, 3, 0, 0, 0, 1, 1, 1] and [int(x) for x in recs["solid"]] == [1, 1, 0, 0, 0, 1, 1, 1]
    assert recs[0]["mean"] == 4 and recs[0]["min_count"] == 2 and recs[0]["max_count"] == 7  # 11 / 3 rounds to 4
    assert M.mean_of(3 * 65535, 3) == 65535 and M.mean_of(5, 2) == 3 and M.mean_of(0, 0) == 0
    assert stats == dict(seqs=8, bytes=len(sb), windows=9, present=9, solid=5, sum=43, longest=10)
    filled = M.kmer_depths(tab, k, sb, offs, fill_mean=True)[0]
    assert (filled[:14] == recs[0]["mean"]).all() and list(filled[14:22]) == [0] * 8 and list(filled[26:35]) == [7, 7, 7, 0, 7, 7, 7, 7, 7]
    assert list(filled[35:45]) == [7, 7, 7, 7, 0, 7, 7, 7, 7, 7]
    empty = M.kmer_depths(tab, k, *M.block([]))
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and empty[2] == dict.fromkeys(M.STATS, 0)
    nothing = M.kmer_depths(tab, k, *M.block(["", ""]))
    assert len(nothing[1]) == 2 and not nothing[1]["windows"].any() and nothing[2] == dict.fromkeys(M.STATS, 0)


def test_spectrum_ties_saturation_and_nothing():
    hist, st = M.spectrum(np.array([5, 5, 3, 3, 9, 65535], dtype=np.uint16))
    assert st == dict(kmers=6, sum_counts=25 + 65535, max_count=65535, mode_count=3, mode_kmers=2, saturated=1)
    assert M.format_spectrum(hist) == "3 2\n5 2\n9 1\n65535 1\n"
    hist, st = M.spectrum(np.zeros(0, dtype=np.uint16))
    assert not hist.any() and len(hist) == M.BINS and st == dict.fromkeys(M.SPECTRUM_STATS, 0) and M.format_spectrum(hist) == ""
