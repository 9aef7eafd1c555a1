"""Forged inputs for kc_local_assm's tests: contigs, paired reads and records placed by hand (a record need not be a true
alignment: the call reads coordinates, never compares a read with its contig)."""
import numpy as np

import depth_model as D
import lassm_model as M
from align_model import revcomp


def genome(seed, n):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), size=n))


class Case:
    def __init__(self, contigs):
        self.contigs = list(contigs)
        self.reads, self.quals, self.rows = [], [], []
        self.means = None

    def read(self, text, qual=None):
        self.reads.append(text)
        self.quals.append(qual)
        return len(self.reads) - 1

    def place(self, r, u, pos, orient=0, score=None):
        """the oriented read R' lies at contig coordinate pos, which may be negative or reach past the contig's end"""
        L, n = len(self.reads[r]), len(self.contigs[u])
        cstart, cstop = max(pos, 0), min(pos + L, n)
        assert cstart < cstop
        self.rows.append(D.rec(r, u, cstart, cstop, rstart=cstart - pos, rstop=cstop - pos, orient=orient, score=score))

    def pair(self, text, u=None, pos=0, orient=0, mate="", qual=None, mate_qual=None, mate_at=None):
        """a pair: the first read with R' = text at pos of contig u (None: no record), the mate as given, placed at
        mate_at = (contig, pos, orient) or not at all"""
        r = self.read(text if orient == 0 else revcomp(text), qual if orient == 0 or qual is None else qual[::-1])
        m = self.read(mate, mate_qual)
        if u is not None:
            self.place(r, u, pos, orient)
        if mate_at is not None:
            self.place(m, *mate_at)
        return r

    def arrays(self):
        alns = D.records(self.rows) if self.rows else np.zeros(0, dtype=D.GAP_ALN_DTYPE)
        _, pairs, _ = D.pair_inserts([len(c) for c in self.contigs], [len(s) for s in self.reads], alns)
        quals = None
        if any(q is not None for q in self.quals):
            quals = [("I" * len(s) if q is None else q) for s, q in zip(self.reads, self.quals)]
        return alns, pairs, quals

    def model(self, k=21, **params):
        alns, pairs, quals = self.arrays()
        return M.local_assm(self.contigs, self.reads, quals, alns, pairs, self.means, k=k, **params)

    def mirrored(self):
        """every contig reverse-complemented, every record flipped with it"""
        alns, pairs, quals = self.arrays()
        c = Case([revcomp(s) for s in self.contigs])
        c.reads, c.quals, c.means = list(self.reads), list(self.quals), self.means
        flipped = M.mirror(self.contigs, [len(s) for s in self.reads], alns)
        c.rows = [tuple(x) for x in flipped.tolist()]
        return c


def new_contigs(block, offsets):
    text = bytes(block).decode()
    return [text[int(offsets[u]):int(offsets[u + 1]) - 1] for u in range(len(offsets) - 1)]


def overhang_case(copies=2, seed=1, ctg=200, start=160, stop=300, **kw):
    """`copies` error-free reads G[start:stop] over the right end of the contig G[0:ctg]"""
    G = genome(seed, stop + 50)
    c = Case([G[:ctg]])
    for _ in range(copies):
        c.pair(G[start:stop], 0, start, **kw)
    return c, G


def haplotype_case():
    """two haplotypes of two reads each that share G[160:250] and diverge there: 50 bases beyond the contig G[0:200]"""
    G = genome(2, 250)
    a, b = genome(3, 60), genome(4, 60)
    b = ("A" if a[0] != "A" else "C") + b[1:]
    c = Case([G[:200]])
    for tail in (a, a, b, b):
        c.pair(G[160:250] + tail, 0, 160)
    return c, G


def repeat_case(rep_len):
    """the contig ends in U R; two reads continue U R V, two reads from elsewhere hold W R Z"""
    U, R, V, W, Z = genome(5, 170), genome(6, rep_len), genome(7, 60), genome(8, 30), genome(9, 60)
    Z = ("A" if V[0] != "A" else "C") + Z[1:]
    W = W[:-1] + ("A" if U[-1] != "A" else "C")
    c = Case([U + R])
    n = len(U) + rep_len
    for _ in range(2):
        c.pair(U[-30:] + R + V, 0, n - rep_len - 30)
        c.pair(W + R + Z, 0, n - rep_len - 30)
    return c, V


def tandem_case():
    unit = genome(10, 30)
    c = Case([genome(11, 100) + unit * 3])
    for _ in range(2):
        c.pair(unit * 5, 0, 100 + 60)
    return c, unit


def random_case(seed, n_ctgs=6, pairs=60, read_len=(1, 140), lower=0.02, n_rate=0.01, qual_mix=True):
    """contigs cut from one genome with gaps between them, reads sampled over it in both orientations with errors, N,
    lower case and mixed qualities; a record for the contig a read overlaps most, mates placed or not"""
    rng = np.random.default_rng(seed)
    G = genome(seed + 1000, 400 * n_ctgs + 200)
    cuts = [(400 * u + 100, 400 * u + 100 + int(rng.integers(0, 260))) for u in range(n_ctgs)]
    c = Case([G[a:b] for a, b in cuts])

    def sample():
        L = int(rng.integers(read_len[0], read_len[1] + 1))
        s = int(rng.integers(0, len(G) - L))
        t = list(G[s:s + L])
        q = []
        for i in range(L):
            x = rng.random()
            if x < n_rate:
                t[i] = "N"
            elif x < n_rate + lower:
                t[i] = t[i].lower()
            elif x < n_rate + lower + 0.01:
                t[i] = "ACGT"[int(rng.integers(0, 4))]
            q.append(chr(33 + int(rng.choice([2, 9, 10, 19, 20, 40], p=[0.03, 0.03, 0.07, 0.07, 0.1, 0.7]))))
        orient = int(rng.integers(0, 2))
        best, at = None, None
        for u, (a, b) in enumerate(cuts):
            ov = min(s + L, b) - max(s, a)
            if ov > 0 and (best is None or ov > best):
                best, at = ov, (u, s - a, orient)
        return "".join(t), "".join(q) if qual_mix else None, at

    for _ in range(pairs):
        t0, q0, at0 = sample()
        t1, q1, at1 = sample()
        if rng.random() < 0.3:
            at1 = None
        if rng.random() < 0.1:
            t1, q1, at1 = "", ("" if qual_mix else None), None
        o0 = at0[2] if at0 else 0
        r = c.read(t0 if o0 == 0 else revcomp(t0), q0 if o0 == 0 or q0 is None else q0[::-1])
        o1 = at1[2] if at1 else 0
        m = c.read(t1 if o1 == 0 else revcomp(t1), q1 if o1 == 0 or q1 is None else q1[::-1])
        if at0:
            c.place(r, *at0)
        if at1:
            c.place(m, *at1)
    c.means = [int(rng.integers(0, 30)) for _ in range(n_ctgs)]
    return c
