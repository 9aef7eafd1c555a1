"""Inputs of tests/cpp/test_driver.cpp that reach the edges of csrc/kcount_driver.hpp, with what the oracle makes of them
(no tests here; tests/test_driver_cases.py and tests/test_gpu_cpp_driver_edges.py use it).

Every builder returns a Case: the program's arguments, its standard input, the oracle's sorted "KMER count L R" dump and
a dict `facts` of what the oracle shows about the input -- the edge the input was built for.  The CPU test asserts the
facts; the GPU test compares the program's dump with `want` line for line and the program's own INFO lines with the
facts that have a counterpart there.  The expectation is always oracle.cpu_oracle: no device, no Python wrapper of the
library.
"""
import functools
import os
import time

import numpy as np

from helpers import random_reads
from oracle import cpu_oracle as O

CAP = 65535
NTHREADS = max(1, min(16, os.cpu_count() or 1))
HASHTABLE_BLOCK_SIZE = 1 << 24  # kcount_driver.hpp: HashTableDriver::HASHTABLE_BLOCK_SIZE
SEQ_BLOCK_SIZE = 3000000        # ParseAndPackDriver::SEQ_BLOCK_SIZE, the reference's KCOUNT_SEQ_BLOCK_SIZE
PROGRAM_MAX_ELEMS = 100000      # what tests/cpp/test_driver.cpp hands to init as max_elems
WIDTH_KS = (31, 32, 63, 64, 95, 96, 125)
SATURATION_COUNTS = (1, 2, 3, 65534, 65535, 65536, 70000)
_COMP_BOTH = str.maketrans("ACGTacgt", "TGCAtgca")


class Case:
    def __init__(self, args, stdin, want, **facts):
        self.args, self.stdin, self.want, self.facts = [str(a) for a in args], stdin, want, facts


def mask(reads, quals, qual_offset=33):
    """kcount.cpp:81-82: a base below the quality cutoff goes in lower-case"""
    return ["".join(c.lower() if ord(x) < qual_offset + 20 else c for c, x in zip(r, q)) for r, q in zip(reads, quals)]


def unmask(masked):
    """the reads and qualities that mask() turns into these lines"""
    return [m.upper() for m in masked], ["".join("#" if c.islower() else "I" for c in m) for m in masked]


def dump(res, k):
    keys, counts, left, right = res
    return sorted("%s %d %s %s" % (O.kmer_to_string(keys[i], k), counts[i], chr(left[i]), chr(right[i])) for i in range(len(counts)))


def genome_of(seed, genome_len):
    """the genome helpers.random_reads draws first from a generator seeded like this"""
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), size=genome_len))


def random_text(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def supermer_facts(o, masked, k):
    """what the sender makes of these reads: supermers and k-mers per target rank, (target, offset in the '_'-joined
    block, length) of every supermer"""
    per_rank, kmers, placed, at = {}, {}, [], 0
    for m in masked:
        for t, st, ln in o.supermers(m):
            per_rank[t] = per_rank.get(t, 0) + 1
            kmers[t] = kmers.get(t, 0) + ln - k - 1
            placed.append((t, at + st, ln))
        at += len(m) + 1
    return per_rank, kmers, placed


def oracle_dump(masked, k, nranks=1, ctgs=()):
    reads, quals = unmask(masked)
    o = O.Oracle(k, nranks=nranks, nthreads=NTHREADS)
    b, q, offs = O.reads_to_arrays(reads, quals)
    o.add_reads(b, q, offs)
    for seq, depth in ctgs:
        o.add_ctg(seq, min(depth, CAP))
    want = dump(o.finalize(), k)
    o.close()
    return want


# ---- 1. widths ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def widths(k, mode):
    """three ranks, reads of k - 4 .. k + 110 bases with Ns and low-quality bases, at the k where the record gains an
    extension word and KmerArray a word"""
    rng = np.random.default_rng(300 + k)
    reads, quals = random_reads(rng, 500, min_len=k - 4, max_len=k + 110, genome_len=3000, n_rate=0.004)
    masked = mask(reads, quals)
    o = O.Oracle(k, nranks=3, nthreads=1)
    per_rank, _, _ = supermer_facts(o, masked, k)
    o.close()
    return Case([k, mode, "ranks=3"], "\n".join(masked) + "\n", oracle_dump(masked, k, nranks=3), supermers_per_rank=per_rank,
                has_n=any("n" in m for m in masked), has_lowq=any(c in m for m in masked for c in "acgt"), words=k // 32 + 1)


# ---- 2. counts in the read pass -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts(k):
    """supermers of k + 19 bases through insert_supermer(packed, c): one per count of SATURATION_COUNTS, and two pairs
    that share their k-mers and differ in the bases around them -- 40000 + 40000 (the count crosses 65535, the
    differing side's extension counters stay below) and 70000 + 70000 (count and both extension counters of either side end at 65535).
    Expected: the oracle's insert_supermer called c times."""
    rng = np.random.default_rng(400 + k)
    items = [(c, random_text(rng, k + 19)) for c in SATURATION_COUNTS]
    for c in (40000, 70000):
        core = random_text(rng, k + 10)
        items += [(c, "A" + core + "C"), (c, "G" + core + "T")]
    o = O.Oracle(k, nranks=1, nthreads=1)
    for c, s in items:
        for _ in range(c):
            o.insert_supermer(0, s)
    _, tcounts, exts = o.dump_table()
    want = dump(o.finalize(), k)
    o.close()
    two_saturated = int(sum(1 for e in exts if (e[:4] == CAP).sum() >= 2 or (e[4:] == CAP).sum() >= 2))
    crossed_below = int(sum(1 for c, e in zip(tcounts, exts) if c == CAP and (e[:4].max() < CAP or e[4:].max() < CAP)))
    return Case([k, "packed"], "".join("=%d %s\n" % it for it in items), want, table_counts=sorted(set(int(c) for c in tcounts)),
                two_saturated=two_saturated, crossed_below=crossed_below, attempted=len(items))


# ---- 3. a flush in the middle of the copies -------------------------------------------------------------------------
def flush_reads():
    """the 400 reads of test_cpp_driver_matches_oracle"""
    rng = np.random.default_rng(77)
    reads, quals = random_reads(rng, 400, min_len=25, max_len=160, genome_len=1500)
    return mask(reads, quals)


@functools.lru_cache(maxsize=None)
def flush(k, path):
    """every read c times, c sized from the bytes P that one round of the reads puts into the driver's buffer so that
    the buffer crosses HASHTABLE_BLOCK_SIZE once: path "packed" through insert_supermer(packed, c) (P counts packed
    bytes), path "ascii" through c calls of insert_supermer_ascii (P counts characters)"""
    masked = flush_reads()
    P = sum(((len(m) + 1) // 2 if path == "packed" else len(m)) + 1 for m in masked)
    c = HASHTABLE_BLOCK_SIZE // P + 2
    reads, quals = unmask(masked)
    b, q, offs = O.reads_to_arrays(reads, quals)
    lens = np.diff(offs)
    offs_c = np.zeros(len(lens) * c + 1, dtype=np.uint64)
    offs_c[1:] = np.cumsum(np.tile(lens, c))
    t0 = time.time()
    o = O.Oracle(k, nranks=16, nthreads=NTHREADS)
    o.add_reads(np.tile(b, c), np.tile(q, c), offs_c)
    res = o.finalize()
    o.close()
    seconds = time.time() - t0
    return Case([k, path, ("count=%d" if path == "packed" else "repeat=%d") % c], "\n".join(masked) + "\n", dump(res, k), round_bytes=P, copies=c,
                total_bytes=P * c, largest_count=int(res[1].max()), reads=len(masked) * c, oracle_seconds=seconds)


def flush_points(masked, copies, path):
    """the driver's buffer over the run, by the header's own condition (insert_supermer's read branch, or
    insert_supermer_ascii called `copies` times a read): (read, copy) before which the buffer is submitted"""
    size, points = 0, []
    for i, m in enumerate(masked):
        item = ((len(m) + 1) // 2 if path == "packed" else len(m)) + 1
        for c in range(copies):
            if size + item >= HASHTABLE_BLOCK_SIZE:
                points.append((i, c))
                size = 0
            size += item
    return points


# ---- 4. the contig pass through the sender --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wire_ctgs(k):
    """reads as in widths(), then contigs as one '_'-joined block through the sender: thirty pieces of the reads' genome,
    a duplicate at another depth, a prefix, a foreign contig, 3000 bases of the genome in one contig, one contig of depth
    65535 and one handed over with 70000 (a count_t; the oracle gets 65535)"""
    seed = 500 + k
    rng = np.random.default_rng(seed)
    reads, quals = random_reads(rng, 500, min_len=k - 4, max_len=k + 110, genome_len=3000, n_rate=0.004)
    genome = genome_of(seed, 3000)
    masked = mask(reads, quals)
    ctgs = []
    for _ in range(30):
        a = int(rng.integers(0, len(genome) - 400))
        ctgs.append((genome[a:a + int(rng.integers(k + 2, 300))], int(rng.integers(1, 50))))
    ctgs += [(ctgs[0][0], ctgs[0][1] + 3), (ctgs[1][0][:len(ctgs[1][0]) // 2], 2), (random_text(rng, 300), 13)]
    ctgs += [(genome, 7), (random_text(rng, 200), CAP), (random_text(rng, 201), 70000)]
    o = O.Oracle(k, nranks=3, nthreads=1)
    per_rank, _, placed = supermer_facts(o, [c for c, _ in ctgs], k)
    long_ranks = sorted(set(t for t, _, _ in o.supermers(genome)))
    long_supermers = len(o.supermers(genome))
    o.close()
    stdin = "\n".join(masked) + "\n" + "".join(">%d %s\n" % (d, c) for c, d in ctgs)
    return Case([k, "wirectg", "ranks=3"], stdin, oracle_dump(masked, k, nranks=3, ctgs=ctgs), reads_only=oracle_dump(masked, k, nranks=3),
                ctg_supermers=len(placed), ctg_supermers_per_rank=per_rank, long_supermers=long_supermers, long_ranks=long_ranks,
                offset_parities=sorted(set(off % 2 for _, off, _ in placed)), length_parities=sorted(set(ln % 2 for _, _, ln in placed)),
                depths=sorted(set(d for _, d in ctgs)))


# ---- 5. the contig block flush --------------------------------------------------------------------------------------
CTG_FLUSH_LEN = 1 << 20
CTG_FLUSH_N = 16


@functools.lru_cache(maxsize=None)
def ctg_flush(k=21):
    """Sixteen contigs of 2^20 characters in one driver: with their separators 2^24 + 16 characters, so ctg_seqs and
    ctg_depths are submitted, cleared and filled again exactly once before the last contig.  Every contig is cut from one
    random genome of 40000 bases read as a circle, from a start of its own and as often round as its length asks, and has a
    depth of its own; so the dump stays at the genome's size although 16.8 M contig k-mers go in.  What a lost, doubled
    or shifted piece would change is carried by three stretches of 200 bases foreign to the genome in every contig, at its
    start, in its middle and at its end: their k-mers are in the dump with that contig's depth and no other."""
    rng = np.random.default_rng(600 + k)
    genome = random_text(rng, 40000)
    reads = [genome[a:a + 100] for a in range(0, 5000, 50)]
    ctgs = []
    for i in range(CTG_FLUSH_N):
        a = int(rng.integers(0, len(genome)))
        body = (genome[a:] + genome * (CTG_FLUSH_LEN // len(genome) + 1))
        own = [random_text(rng, 200) for _ in range(3)]
        half = CTG_FLUSH_LEN // 2
        seq = own[0] + body[:half - 300] + own[1] + body[half - 300:CTG_FLUSH_LEN - 600] + own[2]
        assert len(seq) == CTG_FLUSH_LEN
        ctgs.append((seq, 3 + 2 * i))
    t0 = time.time()
    want = oracle_dump(reads, k, nranks=1, ctgs=ctgs)
    seconds = time.time() - t0
    own_depths = sorted(set(int(l.split()[1]) for l in want))
    stdin = "\n".join(reads) + "\n" + "".join(">%d %s\n" % (d, c) for c, d in ctgs)
    return Case([k, "ctg", "ctg_elems=%d" % (12 << 20)], stdin, want, total_chars=sum(len(c) + 1 for c, _ in ctgs), depths_in_dump=own_depths,
                depths=[d for _, d in ctgs], oracle_seconds=seconds, contigs=len(ctgs))


def ctg_flushes(lengths):
    """how often insert_supermer's contig branch submits a block before the end, by the header's own condition"""
    size, flushes = 0, 0
    for ln in lengths:
        if size and size + 2 * ((ln + 1) // 2) + 1 >= HASHTABLE_BLOCK_SIZE:
            flushes, size = flushes + 1, 0
        size += 2 * ((ln + 1) // 2) + 1
    return flushes


# ---- 6. the reduced buffer ------------------------------------------------------------------------------------------
REDUCED_MEM = 1 << 20


def buffered_occurrences(k, max_elems, gpu_avail_mem):
    """HashTableDriver::init's sizing of the k-mer buffer, restated"""
    words = k // 32 + 1
    buffered = max_elems * 4 + (1 << 20)
    per_kmer = words * 8 * (2.1 if words == 1 else 2.4) + 2.0
    need = buffered * per_kmer
    if gpu_avail_mem and need > 0.8 * gpu_avail_mem:
        buffered = max(int(buffered * (0.8 * gpu_avail_mem / need)), 1 << 16)
    return buffered


@functools.lru_cache(maxsize=None)
def reduced(k):
    """wire mode, three ranks, gpu_avail_mem = 1 MiB: the buffer falls to its floor of 65536 occurrences and at least one
    rank is handed more than that"""
    rng = np.random.default_rng(700 + k)
    reads, quals = random_reads(rng, 3000, min_len=100, max_len=250, genome_len=4000, n_rate=0.002)
    masked = mask(reads, quals)
    o = O.Oracle(k, nranks=3, nthreads=1)
    _, kmers, _ = supermer_facts(o, masked, k)
    o.close()
    return Case([k, "wire", "ranks=3", "mem=%d" % REDUCED_MEM], "\n".join(masked) + "\n", oracle_dump(masked, k, nranks=3), kmers_per_rank=kmers,
                buffered=buffered_occurrences(k, PROGRAM_MAX_ELEMS, REDUCED_MEM), unreduced=buffered_occurrences(k, PROGRAM_MAX_ELEMS, 0))


# ---- 7. one sender over many blocks ---------------------------------------------------------------------------------
def genome_reads(rng, genome, n, min_len, max_len, err=0.01, lowq=0.03):
    """masked reads of both strands of a genome (a numpy array of letters), a read at a time in numpy"""
    out = []
    lens = rng.integers(min_len, max_len + 1, size=n)
    starts = rng.integers(0, len(genome) - max_len, size=n)
    flips = rng.random(n) < 0.5
    for ln, st, flip in zip(lens, starts, flips):
        s = genome[st:st + ln].copy()
        bad = rng.random(ln) < err
        s[bad] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(bad.sum()))
        s[rng.random(ln) < lowq] |= 0x20  # lower-case
        text = s.tobytes().decode()
        out.append(text.translate(_COMP_BOTH)[::-1] if flip else text)
    return out


@functools.lru_cache(maxsize=None)
def reuse(k, mode):
    """the blocks of one ParseAndPackDriver, in this order: k - 1 characters (refused), k, k + 1, k + 2 (one supermer), a
    large block, a small one, 2 999 999 characters -- one below SEQ_BLOCK_SIZE -- cut at read boundaries, and k - 1
    characters again (refused with the members filled).  The segment buffer of the records mode grows at blocks 1 to 4
    and at the largest and is used again at the small one, which the sender writes right after the receivers were handed
    the large one's records."""
    rng = np.random.default_rng(800 + k)
    genome = np.frombuffer(random_text(rng, 3000).encode(), dtype=np.uint8)
    g = genome.tobytes().decode()
    blocks = [[g[:k - 1]], [g[10:10 + k]], [g[20:20 + k + 1]], [g[30:30 + k + 2]], genome_reads(rng, genome, 1500, k - 3, 250),
              genome_reads(rng, genome, 20, k + 2, 120)]
    last, total = [], 0
    for r in genome_reads(rng, genome, 19000, 100, 250):
        if total + len(r) + 1 > SEQ_BLOCK_SIZE - 1 - 100:
            break
        last.append(r)
        total += len(r) + 1
    last.append(g[100:100 + SEQ_BLOCK_SIZE - 1 - total])  # (between 100 and 350 bases)
    blocks.append(last)
    blocks.append([g[40:40 + k - 1]])  # refused once more, now with the largest block's results in the public members
    o = O.Oracle(k, nranks=2, nthreads=1)
    per_block = []
    for b in blocks:
        _, kmers, placed = supermer_facts(o, b, k)
        ln = sum(len(r) for r in b) + len(b) - 1
        per_block.append(dict(len=ln, ok=int(ln >= k), supermers=len(placed), valid=sum(kmers.values()), packed=(ln + 1) // 2))
    o.close()
    cuts = np.cumsum([len(b) for b in blocks])[:-1]
    lines = [r for b in blocks for r in b]
    return Case([k, mode, "ranks=2", "cuts=" + ",".join(str(c) for c in cuts)], "\n".join(lines) + "\n", oracle_dump(lines, k, nranks=2), blocks=per_block)


# ---- 8. bookkeeping -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def move(k):
    """the reads of flush_reads() as packed supermers into a driver that is moved while half of them are buffered"""
    masked = flush_reads()
    return Case([k, "move"], "\n".join(masked) + "\n", oracle_dump(masked, k), attempted=len(masked))
