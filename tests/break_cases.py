"""Forged-record cases for kc_ctg_break, shared by the CPU tests of the model and the GPU tests.  A case
is a list of contigs, the reads' lengths, kc_gap_aln records and kc_pair_rec records, with the call's parameters.  Two ways to
make a weak run exactly where a test wants it:

  run(u, x, r)    disc >= 2 on [x, x + r) of contig u and 1 on the rest of two max_insert windows: an orient-0 mate whose
                  window [x, x + I) begins at x and an orient-1 mate whose window [x + r - I, x + r) ends at x + r; their partners
                  lie on the dump contig (contig 0, too short to have a weak column).  With min_disc = 2 and no spanning pair
                  the weak columns are the run's.
  holes(u, hs)    min_disc = 0 and max_span = 0: spanning pairs cover every column of contig u but the holes, so the weak
                  columns are the interior holes.

T is the scan tile of csrc/kc_break.hpp."""
import functools

import numpy as np

import break_model as M

T = 2048  # BREAK_TILE
NO = M.NO_ALN
GAP_ALN_DTYPE = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("cstart", "<u4"), ("cstop", "<u4"), ("rstart", "<u2"), ("rstop", "<u2"),
                          ("score", "<u4"), ("mismatches", "<u2"), ("seeds", "<u2"), ("orient", "u1"), ("kind", "u1"), ("pad", "u1", (2,))])
PAIR_DTYPE = np.dtype([("aln0", "<u4"), ("aln1", "<u4"), ("insert", "<u4"), ("cls", "u1"), ("pad", "u1", (3,))])
DUMP = 4  # bases of the dump contig, at most 2 * margin in every case: no weak column
DB = DUMP + 1  # its bytes in the block: contig 1 begins at block byte DB


class Case:
    def __init__(self, seed=1, L=8, **kw):
        self.rng = np.random.default_rng(seed)
        self.L = L
        self.contigs, self.read_lens, self.recs, self.prs, self.bulk, self.built = [], [], [], [], [], None
        self.kw = dict(dict(max_insert=64, max_span=0, min_disc=2, margin=4, min_run=1, one_mate=False), **kw)

    # ---- building
    def contig(self, n):
        self.contigs.append("".join("ACGT"[x] for x in self.rng.integers(0, 4, n)))
        return len(self.contigs) - 1

    def rec(self, read, ctg, cstart, cstop, orient=0, rstart=0, rstop=None, kind=0, score=10):
        self.recs.append((read, ctg, cstart, cstop, rstart, cstop - cstart + rstart if rstop is None else rstop, score, 0, 1, orient, kind, (0, 0)))
        return len(self.recs) - 1

    def pair(self, m0=None, m1=None, L0=None, L1=None, cls=0, insert=0):
        """a pair of reads; m0 / m1: None or dict(ctg, cstart, cstop, orient, ...) of the mate's record"""
        r = len(self.read_lens)
        self.read_lens += [self.L if L0 is None else L0, self.L if L1 is None else L1]
        i0 = NO if m0 is None else self.rec(r, **m0)
        i1 = NO if m1 is None else self.rec(r + 1, **m1)
        self.prs.append((i0, i1, insert, cls, (0, 0, 0)))
        return len(self.prs) - 1

    def repeat(self, p, times):
        """pair p, its reads and its records `times` more often (made as arrays, not one by one)"""
        if times > 0:
            self.bulk.append((p, times))

    def dumpmate(self):
        return dict(ctg=0, cstart=0, cstop=DUMP, orient=0)

    def fwd(self, u, s):
        """a whole read forward at s: the window of its partner is [s, s + I)"""
        return dict(ctg=u, cstart=s, cstop=s + self.L, orient=0)

    def rev(self, u, e):
        """a whole read reversed that ends at e: the window of its partner is [e - I, e)"""
        return dict(ctg=u, cstart=e - self.L, cstop=e, orient=1)

    def span(self, u, lo, hi, times=1):
        """proper pairs whose fragment is [lo, hi)"""
        assert self.L <= hi - lo <= self.kw["max_insert"]
        if times:
            self.repeat(self.pair(self.fwd(u, lo), self.rev(u, hi)), times - 1)

    def disc(self, u, at, orient=0, times=1):
        """discordant mates on u whose partners lie on the dump contig; at: s (orient 0) or e (orient 1)"""
        if times:
            self.repeat(self.pair(self.fwd(u, at) if orient == 0 else self.rev(u, at), self.dumpmate()), times - 1)

    def run(self, u, x, r, times=1):
        assert r <= self.kw["max_insert"] and x + r >= self.L and x + self.L <= len(self.contigs[u])
        self.disc(u, x, 0, times)
        self.disc(u, x + r, 1, times)

    def holes(self, u, hs):
        """hs: ascending (position, length) of the stretches no pair spans; every other column is spanned exactly once"""
        n, I = len(self.contigs[u]), self.kw["max_insert"]
        at = 0
        for h, ln in list(hs) + [(n, 0)]:
            g = h - at  # [at, h) in k fragments of L .. I columns
            k = -(-g // I)
            for j in range(k):
                self.span(u, at + g * j // k, at + g * (j + 1) // k)
            at = h + ln

    # ---- the arrays
    def arrays(self):
        """(alns, pairs, read lengths): built once; a test that changes a record copies it first"""
        if self.built is None:
            alns, pairs = np.array(self.recs, dtype=GAP_ALN_DTYPE).reshape(-1), np.array(self.prs, dtype=PAIR_DTYPE).reshape(-1)
            lens = np.array(self.read_lens, dtype=np.uint64)
            for p, times in self.bulk:
                more = np.repeat(pairs[p:p + 1], times)
                first_read, parts = len(lens), []
                for side, name in enumerate(("aln0", "aln1")):
                    i = int(pairs[p][name])
                    if i != NO:
                        r = np.repeat(alns[i:i + 1], times)
                        r["read"] = first_read + 2 * np.arange(times) + side
                        more[name] = len(alns) + sum(len(x) for x in parts) + np.arange(times)
                        parts.append(r)
                alns, pairs = np.concatenate([alns] + parts), np.concatenate((pairs, more))
                lens = np.concatenate((lens, np.tile(lens[2 * p:2 * p + 2], times)))
            self.built = (alns, pairs, lens)
        return self.built

    @property
    def alns(self):
        return self.arrays()[0]

    @property
    def pairs(self):
        return self.arrays()[1]

    @property
    def offsets(self):
        return np.concatenate(([0], np.cumsum(self.arrays()[2]))).astype(np.uint64)

    def contig_block(self):
        text = "".join(c + "_" for c in self.contigs)
        offs = np.concatenate(([0], np.cumsum([len(c) + 1 for c in self.contigs]))).astype(np.uint64)
        return np.frombuffer(text.encode(), dtype=np.uint8).copy(), offs

    def depths(self):
        """a depth per byte of the block that tells the bytes apart, 0 on separators"""
        seqs, _ = self.contig_block()
        d = (np.arange(len(seqs)) % 65521 + 1).astype(np.uint16)
        d[seqs == ord("_")] = 0
        return d

    def model(self, depths=True, **over):
        return M.break_contigs(self.contigs, self.arrays()[2], self.alns, self.pairs, depths=self.depths() if depths else None, **dict(self.kw, **over))


def two(n, runs, seed=1, **kw):
    """the dump contig and one of n - DB - 1 bases: a block of n bytes; runs: (x, r) in the long contig"""
    c = Case(seed, **kw)
    c.contig(DUMP)
    c.contig(n - DB - 1)
    for x, r in runs:
        c.run(1, x, r)
    return c


def size_case(n):
    ln, mg = n - DB - 1, 4
    return two(n, [(mg, 5), (900, 1), (ln - mg - 4, 4)])  # a run at exactly margin, a run of one column, a run ending at len - margin


def tile_last_case():
    return two(3 * T + 1, [(T - 1 - 10 - DB, 11)])  # the run's last column is block byte T - 1


def tile_first_case():
    return two(3 * T + 1, [(T - DB, 9), (2 * T - DB, 1)])  # the runs' first columns are block bytes T and 2T


def three_tiles_case():
    return two(3 * T + 1, [(T - 8 - DB, T + 21)], max_insert=2 * T)  # block bytes [T - 8, 2T + 13): tiles 0, 1 and 2


def cut_tile_first_case():
    return two(3 * T + 1, [(2 * T - DB - 5, 10), (T - DB - 3, 7)])  # m = 2T and m = T as block bytes


def sep_tile_last_case():
    c = Case(2)
    c.contig(DUMP)
    c.contig(T - 1 - DB)  # its separator is block byte T - 1
    c.contig(2 * T)
    c.run(1, T - 1 - DB - 4 - 6, 6)  # ends at len - margin, four bases in front of the separator
    c.run(1, 100, 10)
    c.run(2, 50, 5)
    return c


def margins_case():
    """contigs of 2 * margin and 2 * margin + 1 bases under discordant mates from end to end: one weak column, the middle of the second"""
    c = Case(3)
    c.contig(DUMP)
    for n in (8, 9, 8, 9):
        u = c.contig(n)
        c.disc(u, 0, 0, 2)
    return c


def empties_case():
    c = Case(4)
    c.contig(DUMP)
    c.contig(500)
    for _ in range(300):
        c.contig(0)
    c.contig(700)
    c.run(1, 300, 20)
    c.run(len(c.contigs) - 1, 40, 3)
    c.run(len(c.contigs) - 1, 600, 64)
    return c


def many_case():
    """5000 contigs of 25 to 60 bases around one of 300 020 bases with three breaks; some of the short ones break too"""
    c = Case(5)
    c.contig(DUMP)
    for k in range(5000):
        if k == 2500:
            big = c.contig(300020)
        u = c.contig(int(c.rng.integers(25, 61)))
        if k % 97 == 0:
            c.run(u, 10, 3)
    for x, r in ((5000, 40), (150000, 1), (299000, 64)):
        c.run(big, x, r)
    return c


def saturate_case():
    """65 535, 65 536 and 70 000 identical spanning pairs on three stretches and as many discordant mates on three others: the
    16-bit tracks saturate, the 32-bit counts of the records do not"""
    c = Case(6, one_mate=True, min_disc=65536, max_span=70000)
    c.contig(DUMP)
    u = c.contig(1200)
    for k, n in enumerate((65535, 65536, 70000)):
        c.span(u, 100 + 100 * k, 140 + 100 * k, n)
        c.repeat(c.pair(c.fwd(u, 600 + 100 * k), None), n - 1)
    return c


def levels_case():
    """columns with span 0 .. 4 under disc 3 and disc 0 .. 4 under span 1: max_span and min_disc at, under and over them"""
    c = Case(7, max_insert=32, margin=2)
    c.contig(DUMP)
    u = c.contig(600)
    for k in range(5):
        c.span(u, 20 + 40 * k, 40 + 40 * k, k)
        c.disc(u, 20 + 40 * k, 0, 3)
        c.span(u, 300 + 40 * k, 330 + 40 * k, 1)
        c.disc(u, 300 + 40 * k, 0, k)
    return c


def classes_case():
    """every pair class, both orients, the clamps at both contig ends, an everted pair, a pair one column too long, a mate alone"""
    c = Case(8, L=10, max_insert=40, margin=3, min_disc=1)
    c.contig(DUMP)
    u, v = c.contig(200), c.contig(120)
    c.span(u, 50, 90)  # proper at exactly max_insert
    c.pair(c.fwd(u, 50), c.rev(u, 91))  # one over: both discordant
    c.pair(c.rev(u, 95), c.fwd(u, 65))  # read 0 is the reverse mate: still proper
    c.pair(c.fwd(u, 120), c.rev(u, 125))  # everted: rs < fs
    c.pair(c.fwd(u, 10), c.fwd(u, 30))  # same orient
    c.pair(c.rev(u, 180), c.rev(u, 190))
    c.pair(c.fwd(u, 100), c.rev(v, 60))  # different contigs
    c.pair(dict(ctg=v, cstart=0, cstop=6, orient=0, rstart=4), dict(ctg=v, cstart=14, cstop=20, orient=1, rstart=0, rstop=6))  # fs = -4, a soft end
    c.pair(c.fwd(v, 100), dict(ctg=v, cstart=112, cstop=120, orient=1, rstart=0, rstop=8))  # re = 122 > len
    c.pair(dict(ctg=v, cstart=0, cstop=5, orient=0, rstart=5), c.dumpmate())  # s = -5: [0, 35)
    c.pair(c.dumpmate(), dict(ctg=v, cstart=112, cstop=120, orient=1, rstart=0, rstop=8))  # e = 122: [82, 120)
    c.pair(c.fwd(u, 150), None)  # one mate
    c.pair(None, c.rev(u, 160))
    c.pair(None, None)
    c.pair(None, None, cls=6, insert=77)  # the class and the insert are not read
    c.pair(c.fwd(u, 40), c.rev(v, 50), cls=6, insert=30)  # a forged proper pair across contigs
    return c


def gather_case(n_holes, step=8, seed=9):
    """n_holes one-column holes `step` columns apart in one contig: with step + 1 odd and 16-byte chunks the inserted separators
    meet the chunks at every offset (a hole and its separator: 9 output bytes apart)"""
    c = Case(seed, L=4, max_insert=40, min_disc=0, margin=5)
    c.contig(DUMP)
    u = c.contig(20 + step * n_holes + 33)
    c.holes(u, [(20 + step * k, 1) for k in range(n_holes)])
    return c


def parted_case():
    """reads of one base: runs of 3 and 2 columns parted by one spanned column, runs of min_run - 1 and min_run (4), odd and even"""
    c = Case(11, L=1, max_insert=40, min_disc=0, margin=5, min_run=4)
    c.contig(DUMP)
    u = c.contig(400)
    c.holes(u, [(50, 3), (54, 2), (100, 3), (150, 4), (200, 5), (250, 6), (300, 7)])
    return c


def none_case():
    """contigs and reads, no record at all"""
    c = Case(10)
    c.contig(DUMP)
    c.contig(300)
    for _ in range(5):
        c.pair(None, None)
    return c


BUILDERS = {"size_t-1": lambda: size_case(T - 1), "size_t": lambda: size_case(T), "size_t+1": lambda: size_case(T + 1),
            "size_3t+1": lambda: size_case(3 * T + 1), "tile_last": tile_last_case, "tile_first": tile_first_case, "three_tiles": three_tiles_case,
            "cut_tile_first": cut_tile_first_case, "sep_tile_last": sep_tile_last_case, "margins": margins_case, "empties": empties_case,
            "many": many_case, "saturate": saturate_case, "levels": levels_case, "classes": classes_case, "gather0": lambda: gather_case(0),
            "gather1": lambda: gather_case(1), "gather17": lambda: gather_case(17), "gather4097": lambda: gather_case(4097), "parted": parted_case,
            "none": none_case}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's answer for a case with its own parameters and depths: computed once and shared, never changed"""
    return case(name).model()


# ---- the chain case: a chimeric contig among true ones under noisy pairs (tests/test_gpu_ctg_break_chain.py) --------------
CHAIN_SEED = 20261021
CHAIN_INSERT = 600  # max_insert and margin of the chain's calls: the fragments are 310 .. 490 bases
# 1000 pairs of 400-base fragments over 5000 bases: 80 fragments over an interior column of a true contig.  At the junction only
# the pairs with a read across it span, by the part of that read its record leaves out: a read aligns to the contig that holds
# more than half of it, so about 1000 * 75 / 5000 = 15 pairs from either side, 30 in all.  Half the coverage parts the two.
# About 80 fragments of either genome lie across the junction and have their mates on two contigs: a quarter of that many
# discordant mates is far above what read errors leave in a true contig's interior (none is expected there at all).
CHAIN_KW = dict(max_insert=CHAIN_INSERT, max_span=40, min_disc=20, margin=None, min_run=1, one_mate=False)


@functools.lru_cache(maxsize=None)
def chain_case(seed=CHAIN_SEED, n=5000, pairs=1000, sub_rate=0.01):
    """Two random genomes of n bases.  Contig 0 is chimeric: the left half of the first joined to the right half of the second;
    contigs 1 and 2 are the halves left over, so every base of either genome lies on exactly one contig.  `pairs` pairs from
    either genome, fragments from a clipped N(400, 30), with substitutions as tests/chain_cases.py draws them."""
    import chain_cases as NC
    from links_cases import READ_LEN, genome
    rng = np.random.default_rng(seed)
    GA, GB, h = genome(seed, n), genome(seed + 1, n), n // 2
    reads, quals, truth = [], [], []
    for g, G in enumerate((GA, GB)):
        for _ in range(pairs):
            f = int(np.clip(round(rng.normal(NC.FRAGMENT, 30)), NC.FRAGMENT - 90, NC.FRAGMENT + 90))
            s0 = int(rng.integers(0, n - f - 1))
            pair = [NC.noisy_read(rng, G, s0, False, sub_rate, 0, 0, 0, 0, 0), NC.noisy_read(rng, G, s0 + f - READ_LEN, True, sub_rate, 0, 0, 0, 0, 0)]
            if int(rng.integers(0, 2)):
                pair.reverse()
            for text, q, where in pair:
                reads.append(text)
                quals.append(q)
                truth.append((g,) + where)
    return NC.Case(contigs=[GA[:h] + GB[h:], GA[h:], GB[:h]], reads=reads, quals=quals, truth=truth, junction=h)
