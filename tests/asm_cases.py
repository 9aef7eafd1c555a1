"""Seeded builders of seq blocks for the tests of kc_ctg_select and kc_fasta_text."""
import numpy as np

import asm_model as M

EDGE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 59, 60, 61, 120, 121, 5000)


def random_contig(rng, length, n_rate=0.02):
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=length)
    s[rng.random(length) < n_rate] = ord("N")
    return s.tobytes().decode()


def edge_block(seed=1):
    """Contigs of every length in EDGE_LENGTHS, twice, in a seeded order, Ns scattered through them; the block begins with the
    empty contig and a one-base one and ends with a one-base one and the empty one."""
    rng = np.random.default_rng(seed)
    lengths = list(EDGE_LENGTHS) * 2
    rng.shuffle(lengths)
    lengths = [0, 1] + lengths + [1, 0]
    return M.block([random_contig(rng, l) for l in lengths])


def tiny_block(seed=2):
    """1 001 contigs of 1 .. 3 bases: ids cross 9/10, 99/100 and 999/1000"""
    rng = np.random.default_rng(seed)
    return M.block([random_contig(rng, int(l), 0.1) for l in rng.integers(1, 4, size=1001)])


def small_block():
    """a text under 64 bytes at prefix "s" and width 4"""
    return M.block(["ACGTNAC", "", "GGN", "TTTTACGTA"])


def ties_block(seed=3, n=9000):
    """many equal lengths, over more than one tile of the sort and of the scans"""
    rng = np.random.default_rng(seed)
    return M.block([random_contig(rng, int(l)) for l in rng.integers(20, 28, size=n)])


def n_block():
    """a contig of only N; adjacent contigs that end and begin with N; a run over a whole contig"""
    return M.block(["NNNNN", "ACGTNN", "NNACGT", "N", "N", "ACNGT", "", "NACGN"])


def heavy_lengths(seed, n, cap=20000):
    """min(cap, 21 + floor(200 Pareto(1.2)))"""
    rng = np.random.default_rng(seed)
    return np.minimum(cap, 21 + np.floor(200 * rng.pareto(1.2, size=n))).astype(np.int64)


def scale_block(seed=5, n=100000):
    """n contigs of heavy-tailed lengths, built without a Python loop over the contigs: about 61 MB at the defaults"""
    rng = np.random.default_rng(seed)
    lengths = heavy_lengths(seed + 1, n)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths + 1)
    nbytes = int(offsets[-1])
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=nbytes)]
    seqs[rng.random(nbytes) < 0.001] = ord("N")
    seqs[offsets[1:].astype(np.int64) - 1] = ord("_")
    return seqs, offsets


def parse_fasta(text, prefix):
    """an independent reader of the text: [(id, sequence)]"""
    out = []
    for line in text.decode().split("\n")[:-1]:
        if line.startswith(">"):
            assert line[1:1 + len(prefix)] == prefix
            out.append([int(line[1 + len(prefix):]), ""])
        else:
            out[-1][1] += line
    return [tuple(r) for r in out]
