"""Contigs whose outcome in the contig k-mer pass is known by construction (no tests here; tests/test_ctg_cases.py and
tests/test_gpu_ctg_edges.py use it).  The companion of count_cases.py, whose building block it shares: l + K + r, k + 2
characters.  As a read it holds one k-mer occurrence with both neighbours and no other; so it does as a contig.

A case is one k-mer K, distinct from every other case's k-mer and from their reverse complements, a read side -- a
count_cases flank multiset, possibly empty -- and a list of contig occurrences (left, right, depth, strand).  left and
right are written in K's own frame: an upper-case base, a lower-case base, "N", or None for a contig that ends there
(k + 1 characters: no window has both neighbours, it contributes nothing).  strand "+" shows l + K + r, "-" its reverse
complement.  An occurrence may spell the k-mer it shows with an N in place of a G (N counts as G inside a k-mer, S3) or
with lower-case bases (only a neighbour's case matters): `spell`.

The expectation of a case is computed below from the case alone, in integer Python -- neither the oracle nor the
device is asked:
  * the reads keep K (count >= 2 and both votes a base under dmin_thres): the reads' line, whatever the contigs say;
  * otherwise, every occurrence as the pass sees it (S5: where the shown k-mer is the larger strand, left and
    comp(right) change places; strictly larger, so a palindrome keeps what is shown) carries the same pair of
    upper-case bases, and the smallest depth is at least max(2, dmin_thres): (canonical K, that depth, left, right);
  * otherwise K is absent.
"""
import numpy as np

import count_cases as CC
from count_cases import CAP, COMP, LETTERS, revcomp

GRID_DEPTHS = (0, 1, 2, 3, 4, 5, 6, 19, 20, 21, 65534, 65535)
DMIN_THRES = (1, 2, 3, 5)
READ_SIDES = ("absent", "singleton", "kept", "fork-left", "no-vote-right", "both-missing")
_TEXT_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp_text(s):
    """of a contig as it is written: N stays N, a lower-case base stays lower-case"""
    return s.translate(_TEXT_COMP)[::-1]


def num_words(k):
    """words of a key in the results: the reference's k / 32 + 1 (at k = 32, 64 the last one is all zero)"""
    return k // 32 + 1


def key_of(canon):
    w = CC.pack(canon)
    return w + (0,) * (num_words(len(canon)) - len(w))


class CtgCase:
    def __init__(self, name, family, kmer, reads=(), occs=(), orient="coin", spell=None, **tags):
        self.name, self.family, self.kmer, self.orient, self.tags = name, family, kmer, orient, tags
        self.k = len(kmer)
        self.reads = CC.Case(name, kmer, [list(reads)], orient=orient)
        self.occs = list(occs)
        # how the contigs spell the k-mer they show: None, "N" or "lower", one for all occurrences or one for each
        self.spell = list(spell) if isinstance(spell, (list, tuple)) else [spell] * len(self.occs)
        assert len(self.spell) == len(self.occs)
        self.canon = min(kmer, revcomp(kmer))
        self.key = key_of(self.canon)
        assert all(len(o) == 4 and o[3] in "+-" and 0 <= o[2] <= CAP for o in self.occs)
        assert orient != "given" or (revcomp(kmer) < kmer and all(o[3] == "+" for o in self.occs))

    def contigs(self):
        """[(contig, depth)] of the occurrences"""
        out = []
        for (left, right, depth, strand), how in zip(self.occs, self.spell):
            shown = self.kmer if strand == "+" else revcomp(self.kmer)
            if how == "N":
                j = shown.index("G", 1)
                shown = shown[:j] + "N" + shown[j + 1:]
            elif how == "lower":
                shown = shown[:3].lower() + shown[3:-2] + shown[-2:].lower()
            left, right = (left or "", right or "") if strand == "+" else (revcomp_text(right or ""), revcomp_text(left or ""))
            out.append((left + shown + right, depth))
        return out

    def windows(self):
        """[(left, right, depth)] of the windows with both neighbours, as the pass sees them (a shorter contig has none)"""
        ws = []
        for s, depth in self.contigs():
            if len(s) < self.k + 2:
                continue
            shown = s[1:-1].upper().replace("N", "G")
            left, right = (c if c in LETTERS else "-" for c in (s[0], s[-1]))  # N, lower case: no extension
            if revcomp(shown) < shown:
                left, right = COMP[right], COMP[left]
            ws.append((left, right, depth))
        return ws

    def ctg_result(self, dmin_thres):
        """what the contigs alone leave of K"""
        ws = self.windows()
        if not ws or len({w[:2] for w in ws}) != 1 or "-" in ws[0][:2]:
            return None
        depth = min(w[2] for w in ws)
        if depth < max(2, dmin_thres):
            return None
        return depth, ws[0][0], ws[0][1]

    def result(self, dmin_thres):
        return self.reads.result(dmin_thres) or self.ctg_result(dmin_thres)


def palindrome(k, pick):
    """an even-length k-mer that is its own reverse complement, unused so far"""
    assert k % 2 == 0
    while True:
        h = "".join(LETTERS[i] for i in pick.rng.integers(0, 4, size=k // 2))
        s = h + revcomp(h)
        if s not in pick.used:
            pick.used.add(s)
            return s


def read_side(kind, a, b, c):
    """the flank multiset of a read side; a, b, c: three different letters"""
    return {"absent": [], "singleton": [((a, b), 1)], "kept": [((a, b), 6)], "fork-left": [((a, b), 6), ((c, b), 6)],
            "no-vote-right": [((a, "-"), 6)], "both-missing": [(("-", "-"), 6)]}[kind]


def families(k, seed=1):
    """Every family, over one picker (so that all their k-mers differ).  The cases do not depend on dmin_thres; their
    expectation does."""
    pick = CC.KmerPicker(k, seed)
    cases = []
    n = [0]

    def letters():
        n[0] += 1
        i = n[0]
        return [LETTERS[(i + j) % 4] for j in (0, 1 + i % 3, 1 + (i + 1) % 3)] + [LETTERS[(i // 3) % 4]]

    def add(name, family, occs, kmer=None, **kw):
        cases.append(CtgCase(name, family, kmer or pick(), occs=occs, **kw))

    # read side x one good contig occurrence (its extensions are not the reads')
    for kind in READ_SIDES:
        for strand in "+-":
            a, b, c, d = letters()
            add("reads %s, contig %s" % (kind, strand), "read-side", [(c, d, 7, strand)], reads=read_side(kind, a, b, c), kind=kind)
    # depth grid: one occurrence each
    for depth in GRID_DEPTHS:
        for strand in "+-":
            for kind in ("absent", "singleton"):
                a, b, c, d = letters()
                add("depth %d %s, reads %s" % (depth, strand, kind), "depth-grid", [(c, d, depth, strand)], reads=read_side(kind, a, b, c),
                    depth=depth, kind=kind)
    # two and three occurrences with the same extensions
    for da, db in ((5, 2), (2, 5), (3, 3), (7, 3), (3, 7), (4, 5), (5, 4), (20, 19), (65535, 2), (2, 65535), (65535, 65534), (1, 9), (9, 1),
                   (0, 9), (9, 0)):
        for s1, s2 in ("++", "+-", "--"):
            a, b, _, _ = letters()
            add("depths %d, %d %s%s" % (da, db, s1, s2), "same-exts", [(a, b, da, s1), (a, b, db, s2)], depths=(da, db))
    for ds in ((9, 5, 7), (5, 9, 2), (2, 2, 2), (6, 3, 65535), (4, 4, 1)):
        for ss in ("+-+", "--+"):
            a, b, _, _ = letters()
            add("depths %s %s" % (ds, ss), "same-exts", [(a, b, dp, s) for dp, s in zip(ds, ss)], depths=ds)
    # one occurrence differs: a different base, an N, a lower-case base -- on either side, on either strand
    for what in ("other", "N", "lower"):
        for on in ("left", "right"):
            for s1, s2 in ("++", "+-", "-+"):
                a, b, c, _ = letters()
                odd = {"other": c, "N": "N", "lower": (a if on == "left" else b).lower()}[what]
                second = (odd, b, 9, s2) if on == "left" else (a, odd, 9, s2)
                add("%s %s %s%s" % (what, on, s1, s2), "differs", [(a, b, 9, s1), second], what=what)
            a, b, c, _ = letters()
            if what != "other":  # ... and alone: no occurrence with a base there
                odd = "N" if what == "N" else (a if on == "left" else b).lower()
                add("%s %s alone" % (what, on), "differs", [(odd, b, 9, "+") if on == "left" else (a, odd, 9, "-")], what=what)
    a, b, c, _ = letters()
    add("two agree, the third does not", "differs", [(a, b, 9, "+"), (a, b, 8, "-"), (a, c, 9, "+")], what="other")
    # one on each strand
    for a, b in (("A", "C"), ("G", "G"), ("T", "C")):
        add("each strand, consistent %s%s" % (a, b), "strands", [(a, b, 9, "+"), (a, b, 4, "-")], consistent=True)
        # K's frame (comp(b), comp(a)) on the other strand is SHOWN with a and b, as the first: only the swap tells them apart
        add("each strand, shown alike %s%s" % (a, b), "strands", [(a, b, 9, "+"), (COMP[b], COMP[a], 9, "-")], consistent=False)
    add("each strand, consistent and shown alike", "strands", [("A", "T", 9, "+"), ("A", "T", 5, "-")], consistent=True)
    # K only ever as the larger strand: the swap of sides decides the result
    for i, (occs, reads) in enumerate(((([("A", "C", 9, "+")]), []), ([("A", "C", 9, "+"), ("A", "C", 3, "+")], []),
                                        ([("A", "C", 9, "+"), ("A", "G", 9, "+")], []), ([("N", "C", 9, "+")], []), ([("A", "c", 9, "+")], []),
                                        ([("G", "T", 9, "+")], [(("A", "C"), 1)]), ([("G", "T", 9, "+")], [(("A", "C"), 6)]),
                                        ([("T", "T", 2, "+")], [(("A", "-"), 6)]))):
        add("larger strand %d" % i, "larger-strand", occs, kmer=pick(larger_strand=True), reads=reads, orient="given")
    # even k: K is its own reverse complement; strictly-less keeps what is shown
    if k % 2 == 0:
        add("palindrome, forward alone", "palindrome", [("A", "C", 9, "+")], kmer=palindrome(k, pick), kept=True)
        add("palindrome, other strand alone", "palindrome", [("A", "C", 9, "-")], kmer=palindrome(k, pick), kept=True)
        add("palindrome, both strands, left = comp(right)", "palindrome", [("A", "T", 9, "+"), ("A", "T", 6, "-")], kmer=palindrome(k, pick), kept=True)
        add("palindrome, both strands, G and C", "palindrome", [("G", "C", 3, "-"), ("G", "C", 8, "+")], kmer=palindrome(k, pick), kept=True)
        add("palindrome, both strands, left != comp(right)", "palindrome", [("A", "C", 9, "+"), ("A", "C", 6, "-")], kmer=palindrome(k, pick), kept=False)
        add("palindrome, both strands, equal bases", "palindrome", [("T", "T", 9, "-"), ("T", "T", 9, "+")], kmer=palindrome(k, pick), kept=False)
    # N and lower case inside K
    for strand in "+-":
        for what in ("N", "lower", "N and clean"):
            while True:
                kmer = pick()
                if "G" in kmer[1:-1] and "C" in kmer[1:-1]:  # either strand shows a G that is not its first base
                    break
            a, b, _, _ = letters()
            if what == "N and clean":  # the same k-mer spelled both ways meets itself
                add("inside K: N and clean %s" % strand, "inside", [(a, b, 9, strand), (a, b, 6, "+")], kmer=kmer, spell=["N", None])
            else:
                add("inside K: %s %s" % (what, strand), "inside", [(a, b, 9, strand)], kmer=kmer, spell=what)
    # contigs of k + 1 characters contribute nothing
    a, b, c, _ = letters()
    add("k + 1: no left neighbour", "short", [(None, b, 9, "+")], kept=False)
    add("k + 1: no right neighbour, other strand", "short", [(a, None, 9, "-")], kept=False)
    add("k + 2 and a shallow k + 1 with another base", "short", [(a, b, 9, "+"), (None, c, 1, "+")], kept=True)
    add("k + 2 and k + 1 on the other strand", "short", [(a, None, 0, "-"), (a, b, 8, "-")], kept=True)
    add("k + 1 beside a read singleton", "short", [(a, None, 9, "+")], reads=[((a, b), 1)], kept=False)
    return cases


def seam_cases(k, n, seed=5):
    """n plain cases for a table that takes them in many launches: one occurrence, or two (equal or different right
    neighbours) that the permutation puts far apart; some beside a read singleton, some beside reads that keep K"""
    pick = CC.KmerPicker(k, seed)
    cases = []
    for i in range(n):
        a, b = LETTERS[i % 4], LETTERS[(i // 4) % 4]
        d = 2 + i % 7
        occs = [(a, b, d, "+-"[i % 2])]
        if i % 5 == 1:
            occs.append((a, b, 1 + i % 4, "+-"[(i // 2) % 2]))
        if i % 5 == 3:
            occs.append((a, COMP[b], d, "+"))
        reads = [((b, a), 1)] if i % 11 == 2 else [((b, a), 4)] if i % 11 == 7 else []
        cases.append(CtgCase("seam %d" % i, "seam", pick(), occs=occs, reads=reads))
    return cases


def emit_reads(cases, k, seed):
    """the read sides as count_cases.emit gives them: (bases u8, quals u8, offsets u64)"""
    return CC.emit([c.reads for c in cases], k, seed)


def emit_ctgs(cases, seed=None):
    """(contigs, depths) of every occurrence of every case, in the order of a seeded permutation (None: as built)"""
    ctgs, depths = [], []
    for c in cases:
        for s, d in c.contigs():
            ctgs.append(s)
            depths.append(d)
    if seed is not None:
        order = np.random.default_rng(seed).permutation(len(ctgs))
        ctgs, depths = [ctgs[i] for i in order], [depths[i] for i in order]
    return ctgs, depths


def as_block(ctgs, depths):
    """the same as one '_'-joined block (u8) with the depth of its contig under every byte (u16), separators included"""
    block = np.frombuffer(("_".join(ctgs) + "_").encode(), dtype=np.uint8) if ctgs else np.zeros(0, np.uint8)
    dd = np.zeros(len(block), dtype=np.uint16)
    at = 0
    for c, d in zip(ctgs, depths):
        dd[at:at + len(c) + 1] = d
        at += len(c) + 1
    return block, dd


def expected_results(cases, dmin_thres):
    """the survivors sorted by key: keys (n, k / 32 + 1) u64, counts u16, left u8, right u8 (ASCII)"""
    cs = sorted((c for c in cases if c.result(dmin_thres)), key=lambda c: c.key)
    nl = num_words(cases[0].k)
    keys = np.array([c.key for c in cs], dtype=np.uint64).reshape(-1, nl)
    res = [c.result(dmin_thres) for c in cs]
    return (keys, np.array([r[0] for r in res], dtype=np.uint16), np.array([ord(r[1]) for r in res], dtype=np.uint8),
            np.array([ord(r[2]) for r in res], dtype=np.uint8))


def expected_stats(cases, dmin_thres):
    kept = [c.result(dmin_thres) for c in cases]
    return dict(total_kmers=sum(1 for r in kept if r), sum_counts=sum(r[0] for r in kept if r))


def expected_ctg_stats(cases):
    """(distinct k-mers in the contig table of a single rank, characters submitted): every window with both neighbours
    enters the table, whatever its neighbours are"""
    ctgs, _ = emit_ctgs(cases)
    return sum(1 for c in cases if c.windows()), sum(len(s) + 1 for s in ctgs)
