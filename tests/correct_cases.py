"""The constructions the tests of kc_correct_reads share (tests/correct_model.py); no tests here.

A repeat-free genome, error-free reads tiled over it so that every k-mer of it but the first and the last is counted at least
twice (the first and the last have a dead end and are purged), and reads of it with planted substitutions whose outcome follows
from the rules alone: the plan.  Every planted read lies inside the genome, away from its ends, so each of its error-free
windows is solid at min_count 2; a window with a planted byte is absent, since a random 21-mer or longer does not meet the
genome again (the model tests check that, they do not assume it).  The plan holds at min_windows = 1, where a site at a read's
first or last byte, with its single window, is looked at; min_windows = 2 drops those as THIN.
"""
import numpy as np

import correct_model as M
import kdepth_model as K
from oracle import cpu_oracle as O

MIN_GAIN = 8  # the wrapper's default, which the plans assume
LETTERS = b"ACGT"
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def other_base(rng, c):
    """a letter that c is not, in c's case"""
    up = c & 0xDF
    return rng.choice([x for x in LETTERS if x != up]) | (c & 0x20)


def tiled_reads(G, read_len, step):
    """error-free reads over all of G, each twice"""
    starts = list(range(0, len(G) - read_len, step)) + [len(G) - read_len]
    return [G[s:s + read_len].decode() for s in starts for _ in range(2)]


def genome(k, length, seed):
    """a repeat-free genome in which one (k-1)-mer stands twice, with different neighbours: X at `fork[0]` and at `fork[1]`"""
    def make():
        rng = np.random.default_rng(seed)
        while True:
            g = bytearray(K.unique_genome(rng, length, k))
            p1, p2 = length // 3, 2 * length // 3
            g[p2:p2 + k - 1] = g[p1:p1 + k - 1]
            # the neighbours differ on both sides, so that no k-mer stands twice and none has two extensions
            if g[p1 - 1] == g[p2 - 1] or g[p1 + k - 1] == g[p2 + k - 1]:
                continue
            text = bytes(g)
            seen = set()
            for p in range(length - k + 1):
                w = text[p:p + k]
                rc = K.revcomp(w)
                if w == rc or w in seen or rc in seen:
                    break
                seen.add(w)
            else:
                return text, (p1, p2)
    return cached(("genome", k, length, seed), make)


def counted(k, length=3000, seed=0):
    """(G, the fork's two places, the reads counted as arrays, the oracle's (keys, counts), the model's table)"""
    def make():
        G, fork = genome(k, length, 100 * k + seed)
        reads = tiled_reads(G, k + 60, 30)
        arrays = O.reads_to_arrays(reads)
        (keys, counts, _, _), _ = O.count_reads(reads, None, k=k)
        return G, fork, arrays, (keys, counts), K.table(keys, counts, k)
    return cached(("counted", k, length, seed), make)


def plant(G, at, length, errors, rng, lower=False, n_at=()):
    """a read G[at:at+length] with a wrong base at each of `errors` and an N at each of n_at: (read, truth, [(pos, old, new)])"""
    truth = bytearray(G[at:at + length].lower() if lower else G[at:at + length])
    for p in n_at:
        truth[p] = ord("N")
    read = bytearray(truth)
    for p in errors:
        read[p] = other_base(rng, truth[p])
    return bytes(read), bytes(truth), [(p, read[p], truth[p]) for p in sorted(errors)]


def planted_cases(k):
    """[(name, read, what out is, [(pos, old, new)] the fixes, reasons that stay)] at min_gain 8, min_windows 1, rounds 3"""
    def make():
        G, fork = counted(k)[:2]
        rng = np.random.default_rng(7000 + k)
        ln = 5 * k + 7
        cases = []

        def add(name, got, recovered=True, why=0):
            read, truth, fixes = got
            cases.append((name, read, truth if recovered else read, fixes if recovered else [], why))

        def at(length=ln):  # away from the genome's ends and from the planted repeat
            while True:
                s = int(rng.integers(5, len(G) - length - 5))
                if all(s + length < f - 2 or s > f + k + 2 for f in fork):
                    return s

        for name, p in (("first", 0), ("k-1", k - 1), ("len-k", ln - k), ("last", ln - 1), ("middle", ln // 2)):
            add("one error: " + name, plant(G, at(), ln, [p], rng))
        for d in (1, MIN_GAIN - 1, MIN_GAIN, k - 1, k, 2 * k - 1, 2 * k):
            # between two anchors; closer than min_gain the left site's range ends too early and the run has no right site
            near = d < MIN_GAIN
            add("two errors %d apart" % d, plant(G, at(), ln, [k + 3, k + 3 + d], rng), recovered=not near, why=M.NO_GAIN if near else 0)
        add("error behind an N", plant(G, at(), ln, [2 * k + 1], rng, n_at=[2 * k]))
        add("error in front of an N", plant(G, at(), ln, [2 * k - 1], rng, n_at=[2 * k]))
        add("lower case", plant(G, at(), ln, [k - 1, ln // 2, ln - 1], rng, lower=True))
        for length in (k - 1, k, k + 1, 2 * k, 3 * k, 150):
            j = length // 2  # anchored iff a solid window lies in front of the error's windows or behind them
            anchored = j >= k or j <= length - k - 1
            add("length %d" % length, plant(G, at(length), length, [j] if length > k else [], rng), recovered=anchored or length <= k,
                why=0 if anchored or length <= k else M.UNANCHORED)
        return cases
    return cached(("planted", k), make)


def verdict_cases(k):
    """[(name, read, quals or None, keyword arguments, the reason it must leave)]: nothing is corrected in any of them"""
    def make():
        G, fork = counted(k)[:2]
        rng = np.random.default_rng(8000 + k)
        ln = 4 * k
        s = 40
        deleted = G[s:s + 2 * k] + G[s + 2 * k + 1:s + ln + 1]
        foreign = K.unique_genome(np.random.default_rng(9000 + k), ln, k)
        # ends in the repeated (k-1)-mer and a byte that is neither of the two that follow it in the genome
        p1, p2 = fork
        tail = [x for x in LETTERS if x not in (G[p1 + k - 1], G[p2 + k - 1])][0]
        forked = G[p1 - 2 * k:p1 + k - 1] + bytes([tail])
        near, _, _ = plant(G, s + 200, ln, [2 * k, 2 * k + 1], rng)
        last, _, _ = plant(G, s + 300, ln, [ln - 1], rng)
        mid, _, _ = plant(G, s + 400, ln, [2 * k], rng)
        quals = np.full(ln, 33 + 30, dtype=np.uint8)
        return [("SHORT_RUN", deleted, None, dict(min_windows=1), M.SHORT_RUN),
                ("UNANCHORED", foreign, None, dict(min_windows=1), M.UNANCHORED),
                ("AMBIGUOUS", forked, None, dict(min_windows=1), M.AMBIGUOUS),
                ("NO_GAIN", near, None, dict(min_windows=1), M.NO_GAIN),
                ("THIN", last, None, dict(min_windows=2), M.THIN),
                ("QUAL_GATED", mid, quals, dict(min_windows=1, max_qual=20), M.QUAL_GATED)]
    return cached(("verdicts", k), make)


def block(k, clean=3000):
    """(bases, offsets, the planted cases' first sequence index) of the device tests: see tests/test_gpu_correct_reads.py"""
    def make():
        G, fork = counted(k)[:2]
        rng = np.random.default_rng(6000 + k)
        seqs = [b"", b""]
        first_planted = len(seqs)
        seqs += [c[1] for c in planted_cases(k)]
        seqs += [c[1] for c in verdict_cases(k)]
        seqs += [b""]
        for _ in range(clean):  # a lane sees several sequences and no weak window
            s = int(rng.integers(5, len(G) - k - 30))
            seqs.append(G[s:s + k + int(rng.integers(0, 12))])
        # past a lane's 16 positions, a wave's 1024 and a workgroup's 4096, an error every 170 bytes or so
        for length in (16 + k, 64 * 16 + k, 256 * 16 + k + 3):
            parts, n = [], 0
            while n < length:
                piece = int(rng.integers(2 * k, 400))
                s = int(rng.integers(5, len(G) - piece - 5))
                parts.append(G[s:s + piece])
                n += piece
            text = bytearray(b"".join(parts)[:length])
            for p in range(7, length, 170):
                text[p] = other_base(rng, text[p])
            seqs.append(bytes(text))
        seqs += [b"", G[10:10 + k]]
        b, offs = K.block(seqs)
        return b, offs, first_planted
    return cached(("block", k), make)
