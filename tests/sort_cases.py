"""Result sets known by construction, for the device sort and the device dump text (no tests here;
tests/test_sort_cases.py checks them against the oracle, tests/test_gpu_sort_dump.py runs them on the GPU).

The building block is count_cases.py's: a read a + X + b of exactly k + 2 bases holds one k-mer occurrence with both
neighbours and no other (S5).  All its bases are of high quality and it is submitted c >= 2 times as it stands, so both
votes are unanimous for any c and the one result is canonical(X) with count min(c, 65535), left a, right b.  Every X
here is built to be its own canonical form (X < revcomp(X); `family` asserts it), so the result keys are pack(X) and a
family decides exactly which key bits differ -- which is what a radix sort's passes, digit by digit and word by word,
have to get right.
"""
import numpy as np

from count_cases import LETTERS, pack, revcomp

KS = (21, 31, 32, 33, 64, 77)  # one word; one word with the wider internal record; two words with an all-zero second;
#                                two words; three with an all-zero third; three
CAP = 65535
COUNTS = (2, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535, 70000)  # every digit count, and the clip


def quads():
    return ["".join((LETTERS[(v >> 6) & 3], LETTERS[(v >> 4) & 3], LETTERS[(v >> 2) & 3], LETTERS[v & 3])) for v in range(256)]


def filler(rng, n):
    return "".join(LETTERS[i] for i in rng.integers(0, 4, size=n))


class Family:
    """entries: (X, a, b, c) in the order of submission"""

    def __init__(self, name, k, entries):
        self.name, self.k, self.entries = name, k, entries
        seen = set()
        for x, a, b, c in entries:
            assert len(x) == k and c >= 2 and a in LETTERS and b in LETTERS
            assert x < revcomp(x), (name, x)  # the result key is X itself
            assert x not in seen, (name, x)
            seen.add(x)
        self.short = []  # reads that hold no counted k-mer

    def reads(self):
        out = list(self.short)
        for x, a, b, c in self.entries:
            out.extend([a + x + b] * c)
        return out

    def arrays(self):
        """(bases u8, quals u8, offsets u64), every base of high quality"""
        reads = self.reads()
        offs = np.zeros(len(reads) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        b = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
        return b, np.full(len(b), ord("I"), dtype=np.uint8), offs

    def expected(self):
        """the results in key order: keys (n, words) u64, counts u16, left u8, right u8"""
        es = sorted(self.entries, key=lambda e: pack(e[0]))
        nl = self.k // 32 + 1  # the reference's width: a zero word follows k = 32, 64
        keys = np.zeros((len(es), nl), dtype=np.uint64)
        for i, e in enumerate(es):
            w = pack(e[0])
            keys[i, :len(w)] = w
        return (keys, np.array([min(e[3], CAP) for e in es], dtype=np.uint16), np.array([ord(e[1]) for e in es], dtype=np.uint8),
                np.array([ord(e[2]) for e in es], dtype=np.uint8))


def _flanks(i):
    return LETTERS[i % 4], LETTERS[(i // 4 + i) % 4]


def _entries(xs, rng):
    return [(x,) + _flanks(i) + (int(rng.integers(2, 5)),) for i, x in enumerate(xs)]


def families(k, seed=11):
    """Every family of one k.  A prefix AAAAA (and, where the first bases vary, a suffix AAAAA, whose reverse
    complement starts TTTTT) makes every X smaller than its reverse complement."""
    rng = np.random.default_rng(seed * 1000 + k)
    fams = []
    empty = Family("empty", k, [])
    empty.short = [filler(rng, k + 1), filler(rng, k), filler(rng, 5), "A" * (k + 1)]
    fams.append(empty)
    one = "AAAAA" + filler(rng, k - 6) + "C"
    fams.append(Family("one k-mer", k, [(one, "G", "T", 3)]))
    lo, hi = "AAAAAC" + filler(rng, k - 7) + "C", "AAAAAG" + filler(rng, k - 7) + "C"
    fams.append(Family("two k-mers, the larger first", k, [(hi, "A", "C", 2), (lo, "T", "G", 4)]))
    # the last four bases differ: the lowest digits of the last word, the partial one among them
    p = "AAAAA" + filler(rng, k - 10) + "G"
    xs = [p + v for v in quads()]
    fams.append(Family("low bits", k, _entries([xs[i] for i in rng.permutation(256)], rng)))
    # the first four bases differ: the highest digit of word 0
    s = "A" + filler(rng, k - 10) + "AAAAA"
    xs = [v + s for v in quads()]
    fams.append(Family("high bits", k, _entries([xs[i] for i in rng.permutation(256)], rng)))
    if k >= 33:
        # equal in bases 0..31: word 1 alone decides (k = 33 has one base there)
        h = "AAAAA" + filler(rng, 26) + "C"
        nvar = min(4, k - 32)
        tail = filler(rng, k - 32 - nvar - 1) + "C" if k - 32 - nvar >= 1 else ""
        var = [q[:nvar] for q in quads()[:: 4 ** (4 - nvar)]]
        xs = [h + v + tail for v in var]
        fams.append(Family("word 1 only", k, _entries([xs[i] for i in rng.permutation(len(xs))], rng)))
    if k >= 32:
        # pairs that differ at one base next to the word boundary, and in nothing else
        body = "AAAAA" + filler(rng, k - 6) + "C"
        xs = []
        for pos in (31, 32):
            if pos >= k:
                continue
            for j in range(6):
                b = list("AAAAA" + filler(rng, k - 6) + "C") if j else list(body)
                for c in ("A", "G") if j % 2 else ("T", "C"):
                    b[pos] = c
                    xs.append("".join(b))
        xs = list(dict.fromkeys(xs))
        fams.append(Family("bases 31 and 32", k, _entries([xs[i] for i in rng.permutation(len(xs))], rng)))
    xs = ["AAAAA" + filler(rng, k - 6) + "G" for _ in COUNTS]
    fams.append(Family("counts", k, [(x,) + _flanks(i) + (c,) for i, (x, c) in enumerate(zip(xs, COUNTS))]))
    return fams
