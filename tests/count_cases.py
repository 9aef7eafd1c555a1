"""Reads whose table entry is known by construction (no tests here; tests/test_count_cases.py and
tests/test_gpu_count_edges.py use it).

The building block is a read of exactly k + 2 bases, l + K + r: it holds one k-mer occurrence with both neighbours and
no other (S3: an occurrence needs both).  A case is one random non-palindromic k-mer K, distinct from every other
case's k-mer and from their reverse complements, and a multiset of (left, right) flanks; a flank is A/C/G/T at high
quality or "-" (no extension), which is emitted as N or as a base below the quality cutoff.  Every read is emitted as it
stands or reverse-complemented, by a seeded coin -- except the cases marked orient="given", whose k-mer is the larger of
the two strands and only ever appears that way, so that S5's swap of sides decides the result.

The expectation of a case -- canonical key, count, lc[4], rc[4] (each clipped at 65535), and the result line or "purged"
-- is computed from the flank multiset alone in integer Python below: S5's orientation swap, S6's clip, S7's vote with
D = max((int)((1.0 - 0.9) * count), dmin_thres), S8's purge.  It does not go through spec_model.count_kmers or the
oracle; the tests compare all three.
"""
from collections import Counter

import numpy as np

CAP = 65535
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "-": "-"}
LETTERS = "ACGT"
QUAL_OFFSET = 33
HQ, LQ = chr(QUAL_OFFSET + 40), chr(QUAL_OFFSET + 2)  # the cutoff is qual_offset + 20

GRID_COUNTS = (2, 3, 9, 10, 11, 19, 20, 21, 29, 30, 31, 39, 40, 41, 49, 50, 51, 99, 100, 101, 1000)
SATURATION_NS = (65534, 65535, 65536, 65537, 70000)


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def dmin_dyn(count, dmin_thres):
    """S7's threshold: in double, as the reference computes it (1.0 - 0.9 < 0.1, so this is not count / 10)."""
    return max(int((1.0 - 0.9) * count), dmin_thres)


def pack(kmer):
    """2 bits a base, A C G T = 0 1 2 3, the first base in the top bits of word 0, the last word left-aligned."""
    words = [0] * ((len(kmer) + 31) // 32)
    for i, c in enumerate(kmer):
        words[i // 32] |= LETTERS.index(c) << (2 * (31 - i % 32))
    return tuple(words)


class Case:
    """blocks: per block of reads (submitted separately; most cases have one) a list of ((left, right), n)."""

    def __init__(self, name, kmer, blocks, orient="coin", **tags):
        self.name, self.kmer, self.blocks, self.orient, self.tags = name, kmer, blocks, orient, tags
        rc = revcomp(kmer)
        self.swapped = rc < kmer  # ACGT order is the order of the packed words
        self.canon = rc if self.swapped else kmer
        self.key = pack(self.canon)
        n, lc, rcn = 0, [0] * 4, [0] * 4
        for flanks in blocks:
            for (l, r), m in flanks:
                if self.swapped:  # S5: the other strand's left neighbour is the complement of this one's right
                    l, r = COMP[r], COMP[l]
                n += m
                if l != "-":
                    lc[LETTERS.index(l)] += m
                if r != "-":
                    rcn[LETTERS.index(r)] += m
        self.occurrences = n
        self.count = min(n, CAP)
        self.lc = [min(x, CAP) for x in lc]
        self.rc = [min(x, CAP) for x in rcn]

    def vote(self, c4, dmin_thres):
        top, runner = sorted(c4, reverse=True)[:2]
        d = dmin_dyn(self.count, dmin_thres)
        if top < d:
            return "X"
        if runner >= d:
            return "F"
        return LETTERS[c4.index(top)]  # (top > runner here: a tie is "X" or "F")

    def exts(self, dmin_thres):
        return self.vote(self.lc, dmin_thres), self.vote(self.rc, dmin_thres)

    def result(self, dmin_thres):
        """(count, left, right), or None where S8 purges the k-mer"""
        l, r = self.exts(dmin_thres)
        if self.count < 2 or l in "XF" or r in "XF":
            return None
        return self.count, l, r

    def line(self, dmin_thres):
        res = self.result(dmin_thres)
        return "purged" if res is None else "%s %d %s %s" % ((self.canon,) + res)


class KmerPicker:
    def __init__(self, k, seed):
        self.k, self.rng, self.used = k, np.random.default_rng(seed), set()

    def __call__(self, larger_strand=None):
        """a k-mer no case has used in either orientation; larger_strand True/False: which of its two strands"""
        assert len(self.used) < 4 ** self.k // 2 - 8, "k is too small for this many cases"
        while True:
            s = "".join(LETTERS[i] for i in self.rng.integers(0, 4, size=self.k))
            rc = revcomp(s)
            if s == rc or min(s, rc) in self.used:
                continue
            self.used.add(min(s, rc))
            if larger_strand is None:
                return s
            return max(s, rc) if larger_strand else min(s, rc)


def side(c, top, runner, third, letters):
    """c flanks of one side: `top` of letters[0], `runner` of letters[1], `third` of letters[2], the rest none"""
    assert top + runner + third <= c
    return [letters[0]] * top + [letters[1]] * runner + [letters[2]] * third + ["-"] * (c - top - runner - third)


def pair_up(lefts, rights, shift):
    """the multiset of (left, right) of two sides' flanks; any pairing gives the same entry, `shift` varies it"""
    shift %= max(len(rights), 1)
    cnt = Counter(zip(lefts, rights[shift:] + rights[:shift]))
    return sorted(cnt.items())


def grid_points(c, d):
    """every feasible (top, runner) with top in {D-1, D, D+1} and runner in {0, D-1, D, top}"""
    pts = []
    for top in (d - 1, d, d + 1):
        for runner in sorted({0, d - 1, d, top}):
            if 0 <= runner <= top and top + runner <= c and (top, runner) not in pts:
                pts.append((top, runner))
    return pts


def vote_grid(k, dmin_thres, seed=1):
    """One side on the grid while the other is unanimous (the sides alternate, the letters rotate, the remainder is none
    or a third letter below the runner), a smaller set with both sides on their thresholds, and cases whose k-mer comes
    only as its larger strand."""
    pick = KmerPicker(k, seed)
    cases = []
    i = 0

    def one_side(c, top, runner, with_third):
        third = min(runner - 1, c - top - runner) if with_third and runner >= 2 else 0
        return top, runner, max(third, 0)

    for c in GRID_COUNTS:
        d = dmin_dyn(c, dmin_thres)
        for top, runner in grid_points(c, d):
            i += 1
            t, r, th = one_side(c, top, runner, i % 2 == 0)
            letters = [LETTERS[(i + j) % 4] for j in (0, 1 + i % 3, 1 + (i + 1) % 3)]
            grid = side(c, t, r, th, letters)
            other = [LETTERS[(i // 4) % 4]] * c
            on_left = i % 2 == 1
            flanks = pair_up(grid, other, i) if on_left else pair_up(other, grid, i)
            cases.append(Case("grid c=%d top=%d runner=%d %s" % (c, top, runner, "left" if on_left else "right"), pick(), [flanks],
                              c=c, d=d, top=top, runner=runner, kind="one-side"))
    for c in (30, 40, 50, 100):
        d = dmin_dyn(c, dmin_thres)
        both = [((d, d - 1), (d, d - 1)), ((d, d), (d, 0)), ((d - 1, 0), (d, 0)), ((d, 0), (d - 1, d - 1)), ((d + 1, d - 1), (d, d - 1)),
                ((d, d - 1), (d + 1, d))]
        for (lt, lr), (rt, rr) in both:
            if lt + lr > c or rt + rr > c or lr > lt or rr > rt:
                continue
            i += 1
            lefts = side(c, lt, lr, 0, [LETTERS[i % 4], LETTERS[(i + 1) % 4], "A"])
            rights = side(c, rt, rr, 0, [LETTERS[(i + 2) % 4], LETTERS[(i + 3) % 4], "A"])
            cases.append(Case("both c=%d left=%d/%d right=%d/%d" % (c, lt, lr, rt, rr), pick(), [pair_up(lefts, rights, i)],
                              c=c, d=d, kind="both-sides"))
        # the larger strand only: left is on its threshold and right below it as given, the other way round in the entry
        for (lt, lr), (rt, rr) in (((d, d - 1), (d - 1, 0)), ((d - 1, 0), (d, d - 1)), ((d, d - 1), (c, 0)), ((c, 0), (d, d))):
            if lt + lr > c or rt + rr > c or lr > lt or rr > rt:
                continue
            i += 1
            lefts = side(c, lt, lr, 0, [LETTERS[i % 4], LETTERS[(i + 1) % 4], "A"])
            rights = side(c, rt, rr, 0, [LETTERS[(i + 1) % 4], LETTERS[(i + 3) % 4], "A"])
            cases.append(Case("larger strand c=%d left=%d/%d right=%d/%d" % (c, lt, lr, rt, rr), pick(larger_strand=True),
                              [pair_up(lefts, rights, i)], orient="given", c=c, d=d, kind="larger-strand"))
    return cases


def saturation(k, seed=2, ns=SATURATION_NS):
    """One k-mer with n occurrences, n around 65535, in four flank splits; tags: n, split."""
    pick = KmerPicker(k, seed)
    cases = []
    for j, n in enumerate(ns):
        larger = bool(j % 2)
        cases.append(Case("n=%d A:n-1 C:1" % n, pick(larger), [[(("A", "G"), n - 1), (("C", "T"), 1)]], n=n, split=0))
        cases.append(Case("n=%d A:n-2 C:1 none:1" % n, pick(not larger), [[(("A", "G"), n - 2), (("C", "-"), 1), (("-", "T"), 1)]], n=n, split=1))
        cases.append(Case("n=%d none both sides" % n, pick(larger), [[(("-", "-"), n)]], n=n, split=2))
        cases.append(Case("n=%d left T right none" % n, pick(not larger), [[(("T", "-"), n)]], n=n, split=3))
    return cases


def region_fill(k, n, seed=3):
    """Three k-mers of n / 3 occurrences each: in a geometry of one region the region, not a k-mer, holds n records."""
    pick = KmerPicker(k, seed)
    m = [n // 3, n // 3, n - 2 * (n // 3)]
    return [
        Case("fill 0", pick(False), [[(("A", "C"), m[0])]], n=m[0]),
        Case("fill 1", pick(True), [[(("G", "T"), m[1] - 3), (("C", "T"), 2), (("-", "T"), 1)]], n=m[1]),
        Case("fill 2", pick(), [[(("-", "A"), m[2] - 1), (("T", "A"), 1)]], n=m[2]),
    ]


def two_pass(k, seed=4):
    """Two blocks of reads for a buffer that holds one of them: per-block counts in the names."""
    pick = KmerPicker(k, seed)
    return [
        Case("1+1", pick(), [[(("A", "C"), 1)], [(("A", "C"), 1)]]),
        Case("1+0", pick(), [[(("G", "T"), 1)], []]),
        Case("0+1", pick(), [[], [(("C", "A"), 1)]]),
        Case("32767+32768", pick(False), [[(("A", "G"), 32767)], [(("A", "G"), 32768)]]),
        Case("40000+40000 left A then C", pick(False), [[(("A", "T"), 40000)], [(("C", "T"), 40000)]]),
        Case("65535+1", pick(True), [[(("A", "G"), 65535)], [(("A", "T"), 1)]]),
        Case("30+10 runner 3 in the second", pick(), [[(("A", "G"), 30)], [(("A", "G"), 7), (("C", "G"), 3)]]),
    ]


def emit(cases, k, seed, block=0, shuffle=True):
    """The reads of `block` of the cases: (bases u8, quals u8, offsets u64), every read k + 2 bases long."""
    rng = np.random.default_rng(seed)
    L = k + 2
    rows_b, rows_q = [], []
    for cs in cases:
        if block >= len(cs.blocks):
            continue
        for (l, r), n in cs.blocks[block]:
            # the ways to write this flank pair: "none" as N, or as a base (one that would change the vote) below the cutoff
            tb, tq = [], []
            for lv in ((l, HQ),) if l != "-" else (("N", HQ), (LETTERS[int(rng.integers(0, 4))], LQ)):
                for rv in ((r, HQ),) if r != "-" else (("N", HQ), (LETTERS[int(rng.integers(0, 4))], LQ), ("N", LQ)):
                    fwd, fq = lv[0] + cs.kmer + rv[0], lv[1] + HQ * k + rv[1]
                    tb.append(fwd)
                    tq.append(fq)
                    if cs.orient == "coin":
                        tb.append("".join({"N": "N"}.get(c, COMP.get(c)) for c in reversed(fwd)))
                        tq.append(fq[::-1])
            tb = np.frombuffer("".join(tb).encode(), dtype=np.uint8).reshape(-1, L)
            tq = np.frombuffer("".join(tq).encode(), dtype=np.uint8).reshape(-1, L)
            which = rng.integers(0, len(tb), size=n)
            rows_b.append(tb[which])
            rows_q.append(tq[which])
    if not rows_b:
        return np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    b, q = np.concatenate(rows_b), np.concatenate(rows_q)
    if shuffle:
        order = rng.permutation(len(b))
        b, q = b[order], q[order]
    offs = (np.arange(len(b) + 1, dtype=np.uint64) * np.uint64(L)).astype(np.uint64)
    return np.ascontiguousarray(b).ravel(), np.ascontiguousarray(q).ravel(), offs


def read_strings(bases, quals, k):
    """the same reads as lists of strings (spec_model's input)"""
    L = k + 2
    bs, qs = bases.tobytes().decode(), quals.tobytes().decode()
    return [bs[i:i + L] for i in range(0, len(bs), L)], [qs[i:i + L] for i in range(0, len(qs), L)]


def expected_table(cases):
    """the pre-purge table sorted by key: keys (n, words) u64, counts u16, exts (n, 8) u16 = lc then rc"""
    cs = sorted((c for c in cases if c.occurrences), key=lambda c: c.key)
    nl = len(cs[0].key) if cs else 1
    keys = np.array([c.key for c in cs], dtype=np.uint64).reshape(-1, nl)
    counts = np.array([c.count for c in cs], dtype=np.uint16)
    exts = np.array([c.lc + c.rc for c in cs], dtype=np.uint16).reshape(-1, 8)
    return keys, counts, exts


def expected_results(cases, dmin_thres):
    """the survivors sorted by key: keys, counts u16, left u8, right u8 (ASCII)"""
    cs = sorted((c for c in cases if c.result(dmin_thres)), key=lambda c: c.key)
    nl = len(cases[0].key)
    keys = np.array([c.key for c in cs], dtype=np.uint64).reshape(-1, nl)
    res = [c.result(dmin_thres) for c in cs]
    return (keys, np.array([r[0] for r in res], dtype=np.uint16), np.array([ord(r[1]) for r in res], dtype=np.uint8),
            np.array([ord(r[2]) for r in res], dtype=np.uint8))


def expected_stats(cases, dmin_thres):
    seen = [c for c in cases if c.occurrences]
    kept = [c for c in seen if c.result(dmin_thres)]
    return dict(num_unique=len(seen), num_purged=len(seen) - len(kept), total_kmers=len(kept),
                sum_counts=sum(c.count for c in kept), kmers_inserted=sum(c.occurrences for c in seen))
