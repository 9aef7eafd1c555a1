"""Host model of kc_ctg_index_build / kc_align_reads: a dict index and the candidate and
alignment rules in plain Python, statement by statement.  The reference holds no alignment code, so this file IS the
definition the device is held against; nothing here is shaped after the kernels (no hashing, no packing, no waves).

A block is a str of contigs, every contig followed by '_'; offsets[u] is the start of contig u and offsets[n] the
block's length.  Reads are str; A C G T in either case are bases, anything else is "no base"."""
import numpy as np

MAX_READ_LEN = 1024
KEEP_ALL = 0xFFFFFFFF
COMPLEMENT = str.maketrans("ACGT", "TGCA")
ALN_DTYPE = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("cstart", "<u4"), ("cstop", "<u4"), ("rstart", "<u2"), ("rstop", "<u2"),
                      ("mismatches", "<u2"), ("seeds", "<u2"), ("orient", "u1"), ("pad", "u1", (7,))])
INDEX_STATS = ("contigs", "bases", "windows", "seeds", "repeated")
ALIGN_STATS = ("reads", "reads_aligned", "windows", "seed_hits", "repeated_hits", "alignments", "perfect")


def revcomp(s):
    """Reverse complement of a str over ACGT (any other character stays what it is, reversed)."""
    return s.translate(COMPLEMENT)[::-1]


def join_block(contigs):
    """(block, offsets) of a list of contig strings."""
    offsets, block = [0], []
    for c in contigs:
        block.append(c + "_")
        offsets.append(offsets[-1] + len(c) + 1)
    return "".join(block), offsets


def check_block(block, offsets):
    """None for a block the index takes, else the name of the error it answers with."""
    if any(ch not in "ACGTN_" for ch in block):
        return "KC_ERR_BAD_BASE"
    n = len(offsets) - 1
    if offsets[0] != 0 or offsets[n] != len(block):
        return "KC_ERR_INVALID_ARG"
    seps = [i for i, ch in enumerate(block) if ch == "_"]
    if seps != [offsets[u + 1] - 1 for u in range(n)]:
        return "KC_ERR_INVALID_ARG"
    return None


class Index:
    def __init__(self, block, offsets, k):
        assert check_block(block, offsets) is None
        self.k = k
        self.contigs = [block[offsets[u]:offsets[u + 1] - 1] for u in range(len(offsets) - 1)]
        windows = 0
        found = {}  # canonical k-mer -> every window that has it: (contig, window offset, contig text)
        for u, ctg in enumerate(self.contigs):
            for j in range(len(ctg) - k + 1):
                y = ctg[j:j + k]
                if any(ch not in "ACGT" for ch in y):  # an N is not G here: no window covers it
                    continue
                windows += 1
                rc = revcomp(y)
                key = rc if rc < y else y  # the reverse complement iff it is strictly smaller
                found.setdefault(key, []).append((u, j, y))
        # a seed: exactly one window of the whole block, and not its own reverse complement; else repeated (None)
        self.seeds = {key: (occ[0] if len(occ) == 1 and key != revcomp(key) else None) for key, occ in found.items()}
        self.stats = {"contigs": len(self.contigs), "bases": len(block) - len(self.contigs), "windows": windows,
                      "seeds": sum(1 for v in self.seeds.values() if v is not None),
                      "repeated": sum(1 for v in self.seeds.values() if v is None)}


def align_read(index, read, seed_space, max_mismatches):
    """One read: (records, counters) -- records as tuples (ctg, cstart, cstop, rstart, rstop, mismatches, seeds, orient)
    in the output's order, counters = (windows looked up, seed hits, hits on repeated keys, perfect)."""
    k, L = index.k, len(read)
    assert L <= MAX_READ_LEN and seed_space >= 1
    upper = "".join(ch.upper() if ch in "ACGTacgt" else "." for ch in read)  # '.' = no base
    windows = seed_hits = repeated_hits = perfect = 0
    votes = {}
    for p in range(0, L - k + 1, seed_space):
        w = upper[p:p + k]
        if "." in w:
            continue
        windows += 1
        rc = revcomp(w)
        key = rc if rc < w else w
        if key not in index.seeds:
            continue
        seed = index.seeds[key]
        if seed is None:
            repeated_hits += 1
            continue
        seed_hits += 1
        u, j, y = seed
        if w == y:
            orient, d = 0, j - p
        else:
            assert rc == y
            orient, d = 1, j - (L - k - p)  # the window's place in the reverse-complemented read
        votes[(u, orient, d)] = votes.get((u, orient, d), 0) + 1
    records = []
    for (u, orient, d) in sorted(votes):
        ctg = index.contigs[u]
        rp = upper if orient == 0 else revcomp(upper)
        cstart, cstop = max(0, d), min(len(ctg), d + L)
        rstart, rstop = cstart - d, cstop - d
        mismatches = 0
        for i in range(rstart, rstop):
            if rp[i] == "." or ctg[d + i] == "N" or rp[i] != ctg[d + i]:
                mismatches += 1
        if mismatches <= max_mismatches:
            records.append((u, cstart, cstop, rstart, rstop, mismatches, votes[(u, orient, d)], orient))
            if mismatches == 0 and rstart == 0 and rstop == L:
                perfect += 1
    return records, (windows, seed_hits, repeated_hits, perfect)


def align_reads(index, reads, seed_space=1, max_mismatches=KEEP_ALL):
    """(records as an ALN_DTYPE array, read_first as uint64[nreads + 1], stats dict).  align_read is a pure function of
    the read's text, so equal reads are computed once."""
    done = {}
    rows, read_first = [], []
    st = dict.fromkeys(ALIGN_STATS, 0)
    st["reads"] = len(reads)
    for r, read in enumerate(reads):
        read_first.append(len(rows))
        if read not in done:
            done[read] = align_read(index, read, seed_space, max_mismatches)
        records, (windows, seed_hits, repeated_hits, perfect) = done[read]
        st["windows"] += windows
        st["seed_hits"] += seed_hits
        st["repeated_hits"] += repeated_hits
        st["perfect"] += perfect
        st["alignments"] += len(records)
        st["reads_aligned"] += 1 if records else 0
        for (u, cstart, cstop, rstart, rstop, mismatches, seeds, orient) in records:
            rows.append((r, u, cstart, cstop, rstart, rstop, mismatches, seeds, orient, (0,) * 7))
    read_first.append(len(rows))
    return np.array(rows, dtype=ALN_DTYPE), np.array(read_first, dtype=np.uint64), st
