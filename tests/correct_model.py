"""Host model of kc_correct_reads (include/kcount_mi355_correct.h); no tests here.

The rules are this project's own and this file pins them, over the table kdepth_model.table(...) gives and with its windows:
a window is k bytes that are all A C G T in either case inside one sequence, its count that of its canonical upper-cased text,
solid at max(min_count, 1) or more and weak below.  A weak run is a maximal stretch of weak windows; an anchor is a solid
window right beside it.  Sequences do not see each other, so the model corrects them one by one and puts the call's rounds
together afterwards: a sequence in which a round accepts nothing gives the same sites in every later round.
"""
import numpy as np

import kdepth_model as K

UNANCHORED, SHORT_RUN, THIN, QUAL_GATED, NO_GAIN, AMBIGUOUS = 1, 2, 4, 8, 16, 32
LEFT, RIGHT = 0, 1
MAX_ROUNDS = 8
REC_DTYPE = np.dtype([("weak_before", "<u4"), ("weak_after", "<u4"), ("corrected", "<u2"), ("flags", "<u2"), ("reserved", "<u4")])
FIX_DTYPE = np.dtype([("seq", "<u4"), ("pos", "<u4"), ("old", "u1"), ("new", "u1"), ("round", "u1"), ("side", "u1"), ("score", "<u2"),
                      ("runner_up", "<u2")])
STATS = ("seqs", "bytes", "windows", "weak_before", "weak_after", "sites", "accepted", "rounds")
NON, WEAK, SOLID = 0, 1, 2
_CODE = {c: i for i, c in enumerate(b"ACGT")}


class Counts:
    """the count of a window's text in a table, remembered: the rounds ask for the same windows again and again"""

    def __init__(self, tab):
        self.tab, self.seen = tab, {}

    def __call__(self, window):
        c = self.seen.get(window)
        if c is None:
            c = self.seen[window] = self.tab.get(K.canonical(window), 0)
        return c


def classes(count, k, text, solid_at):
    """NON / WEAK / SOLID for every position of one sequence's text"""
    n = len(text)
    cls = np.zeros(n, dtype=np.uint8)
    if n < k:
        return cls
    base = K._IS_BASE[np.frombuffer(text, dtype=np.uint8)]
    bad = np.concatenate(([0], np.cumsum(~base)))
    for p in np.flatnonzero(bad[k:] == bad[:n - k + 1]):
        cls[p] = SOLID if count(text[p:p + k]) >= solid_at else WEAK
    return cls


def runs(cls):
    """[(a, b, left_anchored, right_anchored)] of the weak runs"""
    weak = np.concatenate(([False], cls == WEAK, [False]))
    solid = np.concatenate(([False], cls == SOLID, [False]))
    first = np.flatnonzero(weak[1:-1] & ~weak[:-2])
    last = np.flatnonzero(weak[1:-1] & ~weak[2:])
    return [(int(a), int(b), bool(solid[a]), bool(solid[b + 2])) for a, b in zip(first, last)]


def sites_of(cls, k):
    """([(e, side, n)] in the order of e, the reasons of the runs that give none)"""
    sites, why = [], 0
    for a, b, left, right in runs(cls):
        n = min(k, b - a + 1)
        if not left and not right:
            why |= UNANCHORED
        elif left and right and b - a + 1 < k:
            why |= SHORT_RUN
        else:
            if left:
                sites.append((a + k - 1, LEFT, n))
            if right and (not left or b - a + 1 >= 2 * k):
                sites.append((b, RIGHT, n))
    return sites, why


def scores(count, k, text, e, side, n, solid_at):
    """{y: score} for the three letters y that byte e is not"""
    x = bytes([text[e]]).upper()
    starts = range(e - k + 1, e - k + 1 + n) if side == LEFT else range(e, e - n, -1)
    out = {}
    for y in b"ACGT":
        if y == x[0]:
            continue
        patched = text[:e] + bytes([y]) + text[e + 1:]
        s = 0
        for p in starts:
            if count(patched[p:p + k]) < solid_at:
                break
            s += 1
        out[y] = s
    return out


def one_round(count, k, text, quals, solid_at, min_gain, min_windows, max_qual, qual_offset):
    """(the sites evaluated, the reasons, [(pos, old, new, side, score, runner_up)], the weak windows) of one sequence's text"""
    cls = classes(count, k, text, solid_at)
    sites, why = sites_of(cls, k)
    evaluated, fixes = 0, []
    for e, side, n in sites:
        if n < min_windows:
            why |= THIN
            continue
        if quals is not None and max_qual > 0 and int(quals[e]) - qual_offset > max_qual:
            why |= QUAL_GATED
            continue
        evaluated += 1
        sc = scores(count, k, text, e, side, n, solid_at)
        ranked = sorted(sc.items(), key=lambda t: -t[1])
        need = min(n, min_gain)
        if ranked[0][1] < need:
            why |= NO_GAIN
        elif ranked[0][1] == ranked[1][1]:
            why |= AMBIGUOUS
        else:
            fixes.append((e, text[e], ranked[0][0] | (text[e] & 0x20), side, ranked[0][1], ranked[1][1]))
    return evaluated, why, fixes, int((cls == WEAK).sum()), int((cls != NON).sum())


def correct_reads(tab, k, bases, offsets, quals=None, min_count=2, min_gain=8, min_windows=2, rounds=3, max_qual=0, qual_offset=33):
    """(out u8, records REC_DTYPE, fixes FIX_DTYPE, stats dict) of the sequences bases[offsets[i]:offsets[i+1]]"""
    assert 1 <= rounds <= MAX_ROUNDS and min_gain >= 1
    count = tab if isinstance(tab, Counts) else Counts(tab)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    n, nbytes = len(offsets) - 1, len(bases)
    out = bases.copy()
    recs = np.zeros(n, dtype=REC_DTYPE)
    stats = dict.fromkeys(STATS, 0)
    if n == 0 or nbytes == 0:
        return out, recs, np.zeros(0, dtype=FIX_DTYPE), stats
    assert int(offsets[0]) == 0 and int(offsets[n]) == nbytes and (np.diff(offsets.astype(np.int64)) >= 0).all()
    solid_at = max(min_count, 1)
    raw = bases.tobytes()
    all_fixes, per_round = [], []  # per_round[i]: the sites evaluated in sequence i, round by round
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        text, q = raw[a:b], None if quals is None else quals[a:b]
        evaluated, corrected = [], 0
        for r in range(1, rounds + 1):
            ev, why, fixes, weak, windows = one_round(count, k, text, q, solid_at, min_gain, min_windows, max_qual, qual_offset)
            if r == 1:
                recs[i]["weak_before"] = weak
                stats["windows"] += windows
            evaluated.append(ev)
            recs[i]["flags"] = why
            if not fixes:
                break
            t = bytearray(text)
            for e, old, new, side, score, runner in fixes:
                t[e] = new
                all_fixes.append((r, i, e, old, new, side, score, runner))
            text = bytes(t)
            corrected += len(fixes)
        else:
            weak = int((classes(count, k, text, solid_at) == WEAK).sum())
        recs[i]["weak_after"] = weak
        recs[i]["corrected"] = min(corrected, 65535)
        out[a:b] = np.frombuffer(text, dtype=np.uint8)
        per_round.append(evaluated)
    # the call's rounds: it stops after the first in which no sequence has a fix; until then every sequence is looked at again
    run = min(rounds, max((f[0] for f in all_fixes), default=0) + 1)
    stats["rounds"] = run
    stats["sites"] = sum(ev[min(r, len(ev)) - 1] for ev in per_round for r in range(1, run + 1))
    all_fixes.sort()
    fx = np.zeros(len(all_fixes), dtype=FIX_DTYPE)
    for j, (r, i, e, old, new, side, score, runner) in enumerate(all_fixes):
        fx[j] = (i, e, old, new, r, side, score, runner)
    stats["seqs"], stats["bytes"], stats["accepted"] = n, nbytes, len(fx)
    stats["weak_before"] = int(recs["weak_before"].astype(np.uint64).sum())
    stats["weak_after"] = int(recs["weak_after"].astype(np.uint64).sum())
    return out, recs, fx, stats
