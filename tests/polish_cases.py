"""Constructions for kc_ctg_polish (tests/polish_model.py): contigs cut from a drawn truth with planted substitutions and N
columns, reads cut from the truth on either strand, and the records that place them -- written down directly, no aligner, so
that every record class and every column class can be hit on purpose and at the tile boundaries of csrc/kc_polish.hpp.

A Case holds contigs, reads, quals (bytes per read, offset 33), the records and the call's keywords.  Everything is drawn from
seeds, built once and shared (cases()); tests must not change what they get."""
import functools
import random

import numpy as np

import depth_model as D

TILE = 1024  # POLISH_TILE
QUAL_OFFSET = 33
COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(COMP)[::-1]


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def other(rng, ch, avoid=""):
    return rng.choice([b for b in "ACGT" if b != ch.upper() and b not in avoid])


class Case:
    def __init__(self, seed, **kw):
        self.rng = random.Random(seed)
        self.truth, self.contigs, self.reads, self.quals, self.rows, self.kw = [], [], [], [], [], kw

    def contig(self, n, errors=(), ns=()):
        """a contig of n bases: its truth, with a substitution at every position of `errors` and an N at every one of `ns`"""
        truth = rand_seq(self.rng, n)
        ctg = list(truth)
        for p in errors:
            ctg[p] = other(self.rng, truth[p])
        for p in ns:
            ctg[p] = "N"
        self.truth.append(truth)
        self.contigs.append("".join(ctg))
        return len(self.contigs) - 1

    def read(self, u, start, L, orient=0, subs=None, lower=(), ns=(), quals=None):
        """a read whose R' lies on contig u's truth from `start` on.  subs: {position of R': base}; lower / ns: positions of R'
        in lower case / as N; quals: the qualities in R's order (default 40).  Returns its index."""
        text = list(self.truth[u][start:start + L])
        assert len(text) == L
        for p, b in (subs or {}).items():
            text[p] = b
        for p in lower:
            text[p] = text[p].lower()
        for p in ns:
            text[p] = "N"
        text = "".join(text)
        q = list(quals) if quals is not None else [40] * L
        assert len(q) == L
        if orient:
            text, q = revcomp(text), q[::-1]
        self.reads.append(text)
        self.quals.append(bytes(x + QUAL_OFFSET for x in q))
        return len(self.reads) - 1

    def place(self, r, u, start, rstart=0, rstop=None, orient=0, times=1, **kw):
        """records of read r on the diagonal `start` of contig u over R'[rstart, rstop)"""
        rstop = len(self.reads[r]) if rstop is None else rstop
        for _ in range(times):
            self.rows.append(D.rec(r, u, start + rstart, start + rstop, rstart, rstop, orient=orient, **kw))

    def cover(self, u, start, L, orient=0, times=1, **kw):
        r = self.read(u, start, L, orient, **kw)
        self.place(r, u, start, orient=orient, times=times)
        return r

    @property
    def alns(self):
        return D.records(self.rows)

    def block(self):
        """(bases uint8, offsets uint64) of the reads, (quals uint8)"""
        offs = np.zeros(len(self.reads) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r) for r in self.reads])
        bases = np.frombuffer("".join(self.reads).encode(), dtype=np.uint8).copy()
        quals = np.frombuffer(b"".join(self.quals), dtype=np.uint8).copy()
        return bases, offs, quals

    def contig_block(self):
        text = "".join(c + "_" for c in self.contigs)
        offs = np.array(D.block_offsets([len(c) for c in self.contigs]), dtype=np.uint64)
        return np.frombuffer(text.encode(), dtype=np.uint8).copy(), offs


def tiles_case():
    """a contig of 2T + 37 bases at the block's start, so that contig positions are block positions: records that start at
    T - 1, T, T - L + 1 and 2T - 1, one 1024-base read across two boundaries, errors on both sides of every boundary; then a
    21-base contig and a 300-base one in the third tile (a separator in mid-tile, two contigs in a tile, a partial last tile)"""
    T, L = TILE, 100
    c = Case(3301, min_depth=3, min_permille=700, max_mismatches=8)
    errors = [0, 5, T - L + 1, T - 2, T - 1, T, T + 1, T + L - 2, 2 * T - 1, 2 * T, 2 * T + 36, 700, 1500]
    u = c.contig(2 * T + 37, errors=errors, ns=[T + 50, 2 * T + 5])
    for start, n in ((0, L), (T - 1, L), (T, L), (T - L + 1, L), (2 * T - 1, 38), (2 * T - 63, L), (650, L), (1450, L)):
        c.cover(u, start, n, times=2)
        c.cover(u, start, n, orient=1, times=1)
    c.cover(u, T - 500, 1024, times=2)
    c.cover(u, T - 500, 1024, orient=1, times=2)
    v = c.contig(21, errors=[0, 20, 7])
    c.cover(v, 0, 21, times=3)
    c.cover(v, 0, 21, orient=1, times=1)
    w = c.contig(300, errors=[0, 150, 299])
    for start in (0, 100, 200, 130):
        c.cover(w, start, 100, times=3)
    return c


def strands_case():
    """orient 1 with uneven qualities on both sides of min_qual, lower-case bases and N in reads, on both strands"""
    c = Case(3302, min_depth=3, min_permille=600, min_qual=20, max_mismatches=8)
    u = c.contig(400, errors=[10, 11, 60, 100, 101, 139, 200, 260, 333], ns=[61, 201])
    rng = c.rng
    for start in range(0, 400 - 70 + 1, 15):
        for orient in (0, 1, 1, 0, 1):
            L = rng.choice((61, 64, 70))
            q = [rng.choice((2, 19, 20, 21, 40)) for _ in range(L)]
            lower = rng.sample(range(L), 6)
            ns = rng.sample(range(L), 2)
            c.cover(u, start, L, orient=orient, quals=q, lower=lower, ns=ns)
    return c


def columns_case():
    """one column a region of 40, every outcome on purpose: min_depth 4, min_permille 750; X is a base that is neither the
    truth's nor the contig's"""
    c = Case(3303, min_depth=4, min_permille=750, max_mismatches=8)
    plans = [("filled", 4, 0, True), ("tie", 2, 2, False), ("at_depth", 4, 0, False), ("below_depth", 3, 0, False),
             ("at_permille", 6, 2, False), ("short_of_permille", 5, 3, False), ("confirmed", 0, 5, False), ("uncovered", 0, 0, False)]
    u = c.contig(40 * len(plans), ns=[40 * i + 17 for i, p in enumerate(plans) if p[3]])
    c.plans = {}
    for i, (name, n_x, n_truth, _) in enumerate(plans):
        col = 40 * i + 17
        x = other(c.rng, c.truth[u][col], avoid=c.contigs[u][col])
        c.plans[name] = (col, x)
        for k in range(n_x):
            c.cover(u, 40 * i + 5, 30, orient=k & 1, subs={12: x})
        for k in range(n_truth):
            # the truth's base at the column, but nothing else: the other columns of these reads are N
            c.cover(u, 40 * i + 5, 30, orient=k & 1, ns=[p for p in range(30) if p != 12])
    return c


def classes_case():
    """every record class: none, filtered, not_best (KC_POLISH_BEST_ONLY), unequal, divergent at max_mismatches + 1 and placed
    at max_mismatches; edge_clip at a contig's end and inside it"""
    c = Case(3304, min_depth=1, min_permille=500, max_mismatches=3, min_score=50, min_len=30, edge_clip=5, best_only=True)
    u = c.contig(500, errors=[2, 40, 497, 250, 255, 300])
    rng = c.rng
    c.cover(u, 0, 60)                 # the left end: not clipped there, clipped inside
    c.cover(u, 440, 60, orient=1)     # the right end
    c.cover(u, 220, 60)               # inside: clipped on both sides
    sub = lambda start, cols: {p: other(rng, c.truth[u][start + p], avoid=c.contigs[u][start + p]) for p in cols}  # noqa: E731
    c.cover(u, 100, 60, subs=sub(100, (7, 20, 33)))          # m = 3: placed
    c.cover(u, 160, 60, subs=sub(160, (7, 20, 33, 50)))      # m = 4: divergent
    r = c.read(u, 280, 60)
    c.place(r, u, 280, score=120)
    c.place(r, u, 280, score=119)                             # not its read's best
    c.place(r, u, 281, score=120)                             # equal score, higher index: not best either
    r = c.read(u, 330, 60)
    c.rows.append(D.rec(r, u, 330, 392, 0, 60, kind=1))       # unequal: 62 contig bases, 60 read bases
    c.rows.append(D.rec(r, u, 330, 360, 0, 30, score=49))     # filtered by score
    c.rows.append(D.rec(r, u, 330, 359, 0, 29, score=100))    # filtered by length
    c.rows.append((r, u, 0, 0, 0, 0, 0, 0, 1, 0, D.KIND_NONE, (0, 0)))  # none
    return c


def deep_case():
    """66 000 records of one 30-base read on one column range: counts saturate at 65535, the decision stays exact"""
    c = Case(3305, min_depth=3, min_permille=1000, max_mismatches=8)
    u = c.contig(100, errors=[40, 55], ns=[41])
    r = c.read(u, 35, 30)
    c.place(r, u, 35, times=66000)
    return c


def long_case():
    """a block of more than 2^16 bytes: the sort takes three radix passes; reads scattered over it on both strands"""
    c = Case(3306, min_depth=2, min_permille=700, max_mismatches=8)
    n = 66000
    rng = c.rng
    spots = sorted(rng.sample(range(0, n - 150, 7), 150))
    u = c.contig(n, errors=[s + 75 for s in spots[::2]], ns=[s + 20 for s in spots[1::5]])
    v = c.contig(500, errors=[250])
    for s in spots:
        c.cover(u, s, 150, orient=rng.randrange(2), times=2)
    c.cover(v, 200, 100, times=2)
    rng.shuffle(c.rows)
    return c


def unplaced_case():
    """records, none of them placed"""
    c = Case(3307, min_depth=1, min_score=1000)
    u = c.contig(200, errors=[50])
    for start in (0, 40, 100):
        c.cover(u, start, 60, times=2)
    return c


def empty_case():
    c = Case(3308)
    c.contig(150, errors=[5], ns=[9])
    c.contig(30)
    c.read(0, 0, 50)
    return c


BUILDERS = {"tiles": tiles_case, "strands": strands_case, "columns": columns_case, "classes": classes_case, "deep": deep_case, "long": long_case,
            "unplaced": unplaced_case, "empty": empty_case}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's answer for a case, computed once"""
    import polish_model as M
    c = case(name)
    return M.polish(c.contigs, c.reads, c.alns, quals=c.quals, qual_offset=QUAL_OFFSET, **c.kw)


# ---- the ground-truth claim's input: a genome, contigs that differ from it by substitutions and N, error-free reads ------------
def genome_case(seed, n=700, L=60, step=5, n_err=7, n_n=2):
    """(genome, contig, reads): reads of L bases every `step` on both strands, all error-free"""
    rng = random.Random(seed)
    genome = rand_seq(rng, n)
    spots = rng.sample(range(30, n - 30, 31), n_err + n_n)
    ctg = list(genome)
    for p in spots[:n_err]:
        ctg[p] = other(rng, genome[p])
    for p in spots[n_err:]:
        ctg[p] = "N"
    reads = []
    for s in range(0, n - L + 1, step):
        reads.append(genome[s:s + L])
        reads.append(revcomp(genome[s:s + L]))
    return genome, "".join(ctg), reads, sorted(spots)
