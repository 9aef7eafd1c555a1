"""CPU proofs for tests/driver_cases.py: every input reaches the edge of csrc/kcount_driver.hpp it was built for, shown
on the oracle's side alone (tests/test_gpu_cpp_driver_edges.py then holds the C++ program against the same cases)."""
import pytest

import driver_cases as D


@pytest.mark.parametrize("k", D.WIDTH_KS)
def test_widths_reach_every_rank_and_word_count(k):
    c = D.widths(k, "wire")
    assert len(c.want) > 50
    assert sorted(c.facts["supermers_per_rank"]) == [0, 1, 2] and min(c.facts["supermers_per_rank"].values()) > 0
    assert c.facts["has_n"] and c.facts["has_lowq"]
    assert D.widths(k, "records").want == c.want and D.widths(k, "records").args[1] == "records"


def test_widths_cover_both_sides_of_every_word_boundary():
    assert [k // 32 + 1 for k in D.WIDTH_KS] == [1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("k", [21, 51])
def test_counts_saturate_in_the_oracle(k):
    c = D.counts(k)
    f = c.facts
    assert 65535 in f["table_counts"] and 65534 in f["table_counts"] and max(f["table_counts"]) == 65535
    assert f["two_saturated"] >= 1  # a vote between two counters that both stand at 65535
    assert f["crossed_below"] >= 1  # 40000 + 40000: the count is clipped, the two extension counters are not
    counts_in_dump = set(int(l.split()[1]) for l in c.want)
    assert counts_in_dump == {2, 3, 65534, 65535}  # (count 1 is purged)
    assert f["attempted"] == len(D.SATURATION_COUNTS) + 4


@pytest.mark.parametrize("k,path", [(21, "packed"), (33, "packed"), (21, "ascii")])
def test_flush_input_crosses_the_block_size_once(k, path):
    c = D.flush(k, path)
    f = c.facts
    assert f["copies"] == D.HASHTABLE_BLOCK_SIZE // f["round_bytes"] + 2
    # more than one block, and no larger than needed for that: under two rounds of the reads above the threshold
    assert D.HASHTABLE_BLOCK_SIZE < f["total_bytes"] < D.HASHTABLE_BLOCK_SIZE + 3 * f["round_bytes"] < 2 * D.HASHTABLE_BLOCK_SIZE
    assert f["largest_count"] > f["copies"] and len(c.want) > 50
    # the one submission before the end falls inside a read's run of copies, not between two reads
    points = D.flush_points(D.flush_reads(), f["copies"], path)
    assert len(points) == 1 and 0 < points[0][1] < f["copies"] - 1
    if path == "packed":
        assert f["round_bytes"] == 18387 and f["copies"] == 914  # seed 77, as the issue measured it


@pytest.mark.parametrize("k", [21, 51, 77, 99])
def test_contigs_through_the_sender_are_cut_by_rank_and_parity(k):
    c = D.wire_ctgs(k)
    f = c.facts
    # the 3000-base contig falls into many supermers: a minimizer of m bases holds for (w + 1) / 2 of the N k-mers in a row
    # on average (w = k - m + 1 windows), and two runs in three change the rank of three: 4 N / (3 (w + 1)) expected (496,
    # 151, 75, 52; the oracle has 530, 156, 84, 45); half of that is asked
    n_kmers, w = 3000 - k - 1, k - min(27, max(15, k * 2 // 3 + 1)) + 1
    assert f["long_ranks"] == [0, 1, 2] and f["long_supermers"] >= 2 * n_kmers // (3 * (w + 1)) >= 26
    assert f["offset_parities"] == [0, 1] and f["length_parities"] == [0, 1]
    assert sorted(f["ctg_supermers_per_rank"]) == [0, 1, 2] and sum(f["ctg_supermers_per_rank"].values()) == f["ctg_supermers"]
    assert 65535 in f["depths"] and 70000 in f["depths"]
    assert len(c.want) > len(f["reads_only"]) > 50  # the contigs added k-mers the reads alone do not keep
    assert sum(1 for l in c.want if l.split()[1] == "65535") >= 2 * (200 - k - 1)  # both saturated contigs are in the dump


def test_contig_flush_input_crosses_the_block_size_once():
    c = D.ctg_flush(21)
    f = c.facts
    assert D.HASHTABLE_BLOCK_SIZE < f["total_chars"] <= D.HASHTABLE_BLOCK_SIZE + f["contigs"]
    assert D.ctg_flushes([D.CTG_FLUSH_LEN] * D.CTG_FLUSH_N) == 1
    assert len(set(f["depths"])) == f["contigs"] and set(f["depths"]) <= set(f["depths_in_dump"])  # every contig shows in the dump
    print("oracle: %.1f s" % f["oracle_seconds"])


@pytest.mark.parametrize("k", [21, 51])
def test_reduced_buffer_is_at_its_floor_and_overflows(k):
    c = D.reduced(k)
    f = c.facts
    assert f["buffered"] == 65536 < f["unreduced"]
    assert max(f["kmers_per_rank"].values()) > 65536 and sorted(f["kmers_per_rank"]) == [0, 1, 2]
    assert len(c.want) > 50


@pytest.mark.parametrize("k", [21, 51])
def test_reuse_blocks_have_the_lengths_the_sender_branches_on(k):
    c = D.reuse(k, "wire")
    b = c.facts["blocks"]
    assert [x["len"] for x in b[:4]] == [k - 1, k, k + 1, k + 2] and b[6]["len"] == D.SEQ_BLOCK_SIZE - 1 and b[7]["len"] == k - 1
    assert [x["ok"] for x in b] == [0, 1, 1, 1, 1, 1, 1, 0]
    assert [x["supermers"] for x in b[:4]] == [0, 0, 0, 1] and [x["valid"] for x in b[:4]] == [0, 0, 0, 1]
    assert b[4]["len"] > b[5]["len"] > b[3]["len"] and b[6]["len"] > b[4]["len"]  # grows, is used again, grows
    assert all(x["supermers"] > 50 for x in b[4:7]) and len(b) == 8
    assert D.reuse(k, "records").want == c.want and len(c.want) > 50
