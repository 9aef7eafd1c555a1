"""Cases for kc_close_gaps whose answer follows from the case alone: a true text cut into contigs with known pieces
missing between them, reads laid over the cuts, the records by geometry (links_cases.geometric_records) and the scaffold
records written down by hand -- nothing here runs kc_scaffold or an aligner.  Used by tests/test_close_model.py (the
model) and tests/test_gpu_close_gaps.py (the device against the model)."""
import numpy as np

import links_cases as LC
from scaffold_model import MEMBER_DTYPE, SCAFFOLD_DTYPE

RC = str.maketrans("ACGTacgt", "TGCAtgca")


def revc(s):
    return s.translate(RC)[::-1]


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


class Case:
    """contigs, reads, alns, scaffolds, members: what the call takes; text: the true text the pieces were cut from"""
    def __init__(self, text, contigs, reads, alns, scaffolds, members):
        self.text, self.contigs, self.reads, self.alns, self.scaffolds, self.members = text, contigs, reads, alns, scaffolds, members

    def args(self):
        return self.contigs, self.reads, self.alns, self.scaffolds, self.members


def scaffold_records(counts, flags=None):
    out, at = np.zeros(len(counts), SCAFFOLD_DTYPE), 0
    for s, c in enumerate(counts):
        out[s] = (at, c, 0, 0, 0, flags[s] if flags else 0, (0, 0))
        at += c
    return out


def build(text, pieces, places, order=None, joins=None, counts=None, touching=None):
    """pieces: (start, stop, reversed) of the members in scaffold order -- reversed: the contig holds the reverse complement,
    so the member's orient is 1; order: the members' contig numbers; joins: the members' old joins (default: the true
    distance where it is positive, else 1: any positive join is a gap); counts: the scaffolds' members (default: one
    scaffold); places: (start, stop, reversed) of the reads; touching: for every read the members it can share bases with
    (default: every member is tried, as links_cases.geometric_records does -- reads times contigs steps)."""
    n = len(pieces)
    order = list(range(n)) if order is None else list(order)
    counts = [n] if counts is None else counts
    heads = set(np.cumsum([0] + list(counts[:-1])).tolist())
    layout = [None] * n
    for i, pc in enumerate(pieces):
        layout[order[i]] = pc
    members = np.zeros(n, MEMBER_DTYPE)
    for i, (a, b, r) in enumerate(pieces):
        j = 0
        if i not in heads:
            j = joins[i] if joins is not None else max(a - pieces[i - 1][1], 1)
        members[i] = (order[i], j, 0, r, (0, 0, 0))
    reads = [revc(text[s:e]) if r else text[s:e] for s, e, r in places]
    if touching is None:
        alns = LC.geometric_records(layout, places)
    else:  # the same records, tried only where they can be: the read's number is put back afterwards
        parts = []
        for i, place in enumerate(places):
            us = sorted(order[m] for m in touching[i])
            part = LC.geometric_records([layout[u] for u in us], [place])
            part["read"], part["ctg"] = i, [us[int(c)] for c in part["ctg"]]
            parts.append(part)
        alns = np.concatenate(parts) if parts else LC.geometric_records(layout, [])
    return Case(text, LC.contigs_of(text, layout), reads, alns, scaffold_records(counts), members)


def two_contigs(g, oa=0, ob=0, la=60, lb=70, seed=1, supporters=3, backward=1, flank=30, order=(0, 1), old_join=None):
    """A and B with g bases missing between them (g < 0: they overlap), `supporters` reads A[-flank:] + fill + B[:flank], the
    last `backward` of them reverse-complemented"""
    rng = np.random.default_rng(seed)
    text = rand_seq(rng, la + g + lb)
    pieces = [(0, la, oa), (la + g, la + g + lb, ob)]
    lo, hi = (la - flank, la + g + flank) if g >= 0 else (la + g - flank, la + flank)
    places = [(lo, hi, 1 if i >= supporters - backward else 0) for i in range(supporters)]
    joins = None if old_join is None else [0, old_join]
    return build(text, pieces, places, order=order, joins=joins)


def chain(n, seed=1, gaps=(1, 12), lens=(40, 80), per_join=2, flank=25, flip=False, reorder=None):
    """n contigs of one scaffold with a positive gap at every join and per_join reads across each, contig numbers shuffled,
    strands random; flip: every contig reverse-complemented, reorder: another shuffle of the numbers -- the text is the same"""
    rng = np.random.default_rng(seed)
    ls = rng.integers(lens[0], lens[1], size=n).tolist()
    gs = rng.integers(gaps[0], gaps[1], size=n - 1).tolist() if n > 1 else []
    text = rand_seq(rng, sum(ls) + sum(gs))
    pieces, places, touching, at = [], [], [], 0
    for i in range(n):
        if i:
            for q in range(per_join):
                places.append((at - flank, at + gs[i - 1] + flank, (i + q) & 1))
                touching.append((i - 1, i))
            at += gs[i - 1]
        pieces.append((at, at + ls[i], int(rng.integers(0, 2))))
        at += ls[i]
    order = rng.permutation(n).tolist()
    if flip:
        pieces = [(a, b, r ^ 1) for a, b, r in pieces]
    if reorder is not None:
        order = np.random.default_rng(reorder).permutation(n).tolist()
    return build(text, pieces, places, order=order, touching=touching)


def hand_case(A, B, fills, old_join=9, backward=(), flank=30, extra_contigs=()):
    """contigs A and B as they stand, one scaffold A -> B with an N run of old_join, and a read A[-flank:] + fill + B[:flank]
    for every fill (any bytes, any length), read i reverse-complemented for i in backward; the records by hand"""
    from depth_model import rec, records
    reads, rows = [], []
    for i, f in enumerate(fills):
        t = A[-flank:] + f + B[:flank]
        o = 1 if i in backward else 0
        reads.append(revc(t) if o else t)
        rows.append(rec(i, 0, len(A) - flank, len(A), rstart=0, rstop=flank, orient=o))
        rows.append(rec(i, 1, 0, flank, rstart=flank + len(f), rstop=2 * flank + len(f), orient=o))
    n = 2 + len(extra_contigs)
    members = np.zeros(n, MEMBER_DTYPE)
    members[0] = (0, 0, 0, 0, (0, 0, 0))
    members[1] = (1, old_join, 0, 0, (0, 0, 0))
    for i in range(2, n):
        members[i] = (i, 0, 0, 0, (0, 0, 0))
    return Case(None, [A, B] + list(extra_contigs), reads, records(rows), scaffold_records([2] + [1] * (n - 2)), members)
