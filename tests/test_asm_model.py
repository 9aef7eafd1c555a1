"""tests/asm_model.py against expectations written out by hand, and its text against an independent reader (no GPU needed)."""
import numpy as np
import pytest

import asm_cases as AC
import asm_model as M

THREE = ["ACGTACGTAC", "", "NNACG"]


def test_three_contigs_at_width_0_and_4():
    seqs, offsets = M.block(THREE)
    assert bytes(seqs) == b"ACGTACGTAC__NNACG_" and list(offsets) == [0, 11, 12, 18]
    assert M.fasta(seqs, offsets, None, "scaffold_", 0) == b">scaffold_0\nACGTACGTAC\n>scaffold_1\n\n>scaffold_2\nNNACG\n"
    assert M.fasta(seqs, offsets, None, "c", 4) == b">c0\nACGT\nACGT\nAC\n>c1\n\n>c2\nNNAC\nG\n"
    assert M.fasta(seqs, offsets, [2, 0, 2], "", 5) == b">2\nNNACG\n>0\nACGTA\nCGTAC\n>2\nNNACG\n"
    assert M.fasta(seqs, offsets, [], "c", 4) == b""


@pytest.mark.parametrize("width", (0, 1, 15, 16, 17, 60))
def test_record_bytes_is_the_size_of_a_record(width):
    seqs, offsets = AC.edge_block()
    for prefix in ("", "scaffold_"):
        for u, c in enumerate(M.contigs(seqs, offsets)):
            assert len(M.record(u, c, prefix, width)) == M.record_bytes(u, len(c), len(prefix), width)
    assert M.record_bytes(1000, 0, 3, width) == 1 + 3 + 4 + 1 + 0 + 1


def test_n50_and_n90_of_the_example():
    seqs, offsets = M.block(["A" * l for l in (40, 80, 20, 70, 30, 50)])
    order, st = M.select(seqs, offsets, 0, True)
    assert order == [1, 3, 5, 0, 4, 2]
    assert (st["n50"], st["l50"], st["n90"], st["l90"]) == (70, 2, 30, 5)
    assert (st["longest"], st["shortest"], st["key_bits"], st["selected"], st["sel_bases"]) == (80, 20, 6, 6, 290)
    assert M.nx([80, 70, 50, 40, 30, 20], 50) == (70, 2) and M.nx([80, 70, 50, 40, 30, 20], 90) == (30, 5)
    assert M.nx([10, 10], 50) == (10, 1) and M.nx([0, 0], 50) == (0, 1) and M.nx([], 50) == (0, 0)
    # min_len at a present length and one above it
    assert M.select(seqs, offsets, 50, False)[0] == [1, 3, 5] and M.select(seqs, offsets, 51, False)[0] == [1, 3]


def test_an_empty_selection_and_a_single_contig():
    seqs, offsets = M.block(THREE)
    order, st = M.select(seqs, offsets, 11, True)
    assert order == [] and st["contigs"] == 3 and st["bases"] == 15
    assert all(st[k] == 0 for k in M.STATS if k not in ("contigs", "bases", "ge_count", "ge_bases")) and st["ge_count"] == st["ge_bases"] == [0] * 5
    order, st = M.select(*M.block(["ACGTN"]), 0, True)
    assert order == [0] and (st["n50"], st["l50"], st["n90"], st["l90"], st["longest"], st["shortest"], st["key_bits"]) == (5, 1, 5, 1, 5, 5, 0)
    assert (st["a"], st["c"], st["g"], st["t"], st["n"], st["n_runs"]) == (1, 1, 1, 1, 1, 1)
    order, st = M.select(*M.block([]), 0, True)
    assert order == [] and st["contigs"] == st["selected"] == 0
    order, st = M.select(*M.block([""]), 0, False)
    assert order == [0] and (st["selected"], st["sel_bases"], st["l50"], st["n50"]) == (1, 0, 1, 0)


def test_runs_of_n_across_a_contig_boundary():
    seqs, offsets = M.block(["ACNN", "NNGT", "N", "ANNA"])
    assert M.select(seqs, offsets, 0, False)[1]["n_runs"] == 4  # the '_' between them is no N
    assert M.select(seqs, offsets, 4, False)[1]["n_runs"] == 3 and M.select(seqs, offsets, 4, False)[1]["n"] == 6
    assert M.select(seqs, offsets, 5, False)[1]["n_runs"] == 0


def test_ties_in_length_keep_block_order():
    seqs, offsets = M.block(["AC", "ACG", "GT", "TTT", "A", "CC"])
    assert M.select(seqs, offsets, 0, True)[0] == [1, 3, 0, 2, 5, 4]
    assert M.select(seqs, offsets, 2, True)[0] == [1, 3, 0, 2, 5] and M.select(seqs, offsets, 2, False)[0] == [0, 1, 2, 3, 5]


def test_classes():
    seqs, offsets = M.block(["A" * l for l in (999, 1000, 5000, 50000)])
    st = M.select(seqs, offsets, 0, False)[1]
    assert M.CLASSES == (1000, 5000, 10000, 25000, 50000)
    assert st["ge_count"] == [3, 2, 1, 1, 1] and st["ge_bases"] == [56000, 55000, 50000, 50000, 50000]


@pytest.mark.parametrize("width", (0, 1, 15, 16, 17, 60))
def test_an_independent_reader_gets_the_selected_contigs_back(width):
    seqs, offsets = AC.edge_block()
    ctgs = [c.decode() for c in M.contigs(seqs, offsets)]
    for min_len, by_length in ((0, False), (16, True), (61, True)):
        order, _ = M.select(seqs, offsets, min_len, by_length)
        text = M.fasta(seqs, offsets, order, "scaffold_", width)
        assert AC.parse_fasta(text, "scaffold_") == [(u, ctgs[u]) for u in order]
        assert all(len(line) <= width for line in text.decode().split("\n") if width and not line.startswith(">"))


def test_windows():
    text = M.fasta(*AC.small_block(), None, "s", 4)
    assert b"".join(M.window(text, i, 1) for i in range(len(text) + 1)) == text
    assert M.window(text, len(text), 5) == b"" and M.window(text, 3, 10 ** 6) == text[3:]
    with pytest.raises(ValueError):
        M.window(text, len(text) + 1, 1)


def test_the_scale_block_is_what_it_says():
    lengths = AC.heavy_lengths(6, 100000)
    assert lengths.min() >= 21 and lengths.max() == 20000 and 55e6 < int(lengths.sum()) < 70e6
    seqs, offsets = AC.scale_block(n=2000)
    assert (np.diff(offsets.astype(np.int64)) - 1 == AC.heavy_lengths(6, 2000)).all()
    assert (seqs[offsets[1:].astype(np.int64) - 1] == ord("_")).all() and set(bytes(seqs)) <= set(b"ACGTN_")
