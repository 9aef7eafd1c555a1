"""Host model of kc_local_assm (csrc/kc_lassm.hpp): the rules of include/kcount_mi355.h and DESIGN.md section 18 in plain
Python, statement by statement -- dicts for the tables, lists for the texts, no hashing, no waves.  The reference holds no
local assembly (no localassm in src/; src/contigging.cpp:167-172 is commented out), so this file IS the definition the
device is compared with, byte for byte; tests/test_lassm_model.py checks it against cases whose answer follows from the
case alone.

Contigs and reads are str as in tests/align_model.py; quals are str of the same lengths (or None: every base is high
quality); records are GAP_ALN_DTYPE arrays, pairs PAIR_DTYPE arrays as depth_model.pair_inserts returns them."""
import numpy as np

from depth_model import PAIR_DTYPE, NO_ALN, MAX_READ_LEN, INSERT_MAX, BadArg, BadRead, BadRecord, check_records  # noqa: F401
from gap_model import GAP_ALN_DTYPE, KIND_NONE  # noqa: F401

MAX_MER_LEN = 128
MAX_WALK = 4096
MAX_CANDS = 1 << 20
NO_CANDS, TOO_MANY, DEAD_END, FORK, LOOP, MAX_LEN = range(6)
LASSM_END_DTYPE = np.dtype([("cands", "<u4"), ("ext_len", "<u4"), ("out_pos", "<u4"), ("iters", "<u2"), ("mer_len", "u1"), ("status", "u1")])
LASSM_STATS = ("ends", "status", "cands_overhang", "cands_mate", "cand_bases", "iterations", "ext_bases", "ctgs_extended")
DEFAULTS = dict(min_mer_len=13, max_mer_len=121, shift=8, max_walk_len=400, max_insert=1000, min_qual=10, hi_qual=20, min_viable=2,
                viable_permille=200, max_cands=2000, table_budget_mb=0, flags=0)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
HI, LO, NONE = 2, 1, 0


class BadPair(ValueError):
    """an invalid pair record: .index is the lowest bad index"""
    def __init__(self, index):
        ValueError.__init__(self, "pair %d" % index)
        self.index = index


def check_params(p):
    """the ranges kc_local_assm checks in front of the context"""
    if not 4 <= p["min_mer_len"] <= p["max_mer_len"] <= MAX_MER_LEN or not 1 <= p["shift"] <= 64:
        raise BadArg("mer lengths")
    if not 1 <= p["max_walk_len"] <= MAX_WALK:
        raise BadArg("max_walk_len")
    if not 1 <= p["max_insert"] <= INSERT_MAX:
        raise BadArg("max_insert")
    if not p["min_qual"] <= p["hi_qual"] <= 93:
        raise BadArg("qualities")
    if p["min_viable"] < 1 or p["viable_permille"] > 1000:
        raise BadArg("viable")
    if not 1 <= p["max_cands"] <= MAX_CANDS:
        raise BadArg("max_cands")
    if p["flags"]:
        raise BadArg("flags")


def codes_of(text):
    return [CODE.get(ch, 4) for ch in text]


def classes_of(qual, n, p, qual_offset):
    if qual is None:
        return [HI] * n
    out = []
    for ch in qual:
        q = ord(ch) - qual_offset
        out.append(HI if q >= p["hi_qual"] else LO if q >= p["min_qual"] else NONE)
    return out


def revcomp_codes(codes, classes):
    return [c if c == 4 else 3 - c for c in reversed(codes)], list(reversed(classes))


def check_pairs(pairs, alns, nreads):
    for i in range(nreads // 2):
        for side, name in ((0, "aln0"), (1, "aln1")):
            a = int(pairs[i][name])
            if a == NO_ALN:
                continue
            if not (a < len(alns) and int(alns[a]["read"]) == 2 * i + side and int(alns[a]["kind"]) != KIND_NONE):
                raise BadPair(i)


def candidates(contigs, reads, quals, alns, pairs, p, qual_offset):
    """per end (2u: left, 2u + 1: right) the list of (codes, classes, is_mate) of its candidates, in read order"""
    ends = [[] for _ in range(2 * len(contigs))]

    def best(r):
        a = int(pairs[r >> 1]["aln%d" % (r & 1)])
        return None if a == NO_ALN else alns[a]

    def text(r, rc):
        c, q = codes_of(reads[r]), classes_of(None if quals is None else quals[r], len(reads[r]), p, qual_offset)
        return revcomp_codes(c, q) if rc else (c, q)

    for r in range(len(reads)):
        L, b = len(reads[r]), best(r)
        if L == 0 or b is None:
            continue
        u, orient = int(b["ctg"]), int(b["orient"])
        len_u = len(contigs[u])
        ps = int(b["cstart"]) - int(b["rstart"])
        pe = int(b["cstop"]) + (L - int(b["rstop"]))
        # R' is the read in contig orientation: the reverse complement iff orient is 1
        if pe > len_u:
            ends[2 * u + 1].append(text(r, orient == 1) + (False,))
        if ps < 0:
            ends[2 * u].append(text(r, orient == 0) + (False,))
        m = r ^ 1
        bm = best(m)
        unplaced = len(reads[m]) > 0 and (bm is None or int(bm["ctg"]) != u)
        if unplaced and orient == 0 and ps + p["max_insert"] > len_u:
            ends[2 * u + 1].append(text(m, True) + (True,))
        if unplaced and orient == 1 and pe - p["max_insert"] < 0:
            ends[2 * u].append(text(m, True) + (True,))
    return ends


def build_table(cands, m):
    """mer (tuple of codes) -> [hi[4], lo[4]]"""
    table = {}
    for codes, classes, _ in cands:
        n = len(codes)
        for pos in range(n - m):  # pos + m < n
            w = codes[pos:pos + m]
            e = codes[pos + m]
            if 4 in w or e == 4 or classes[pos + m] == NONE:
                continue
            t = table.setdefault(tuple(w), [[0] * 4, [0] * 4])
            t[0 if classes[pos + m] == HI else 1][e] += 1
    return table


def walk(table, S, ext, m, thr, max_walk_len):
    """one iteration: appends to ext, returns the status that ends it"""
    visited = set()
    while True:
        cur = S + ext
        if len(cur) < m:
            return DEAD_END
        M = tuple(cur[-m:])
        if 4 in M or M not in table:
            return DEAD_END
        if M in visited:
            return LOOP
        visited.add(M)
        hi, lo = table[M]
        viable = [b for b in range(4) if hi[b] + lo[b] >= thr and hi[b] >= 1]
        if not viable:
            return DEAD_END
        if len(viable) >= 2:
            return FORK
        ext.append(viable[0])
        if len(ext) == max_walk_len:
            return MAX_LEN


def extend_end(tail, cands, k, mean, p):
    """(ext codes, status, iters, mer_len) of one end with at least one and at most max_cands candidates"""
    thr = max(p["min_viable"], p["viable_permille"] * mean // 1000)
    m = min(max(k, p["min_mer_len"]), p["max_mer_len"])
    ext, iters, last = [], 0, 0  # last: +1 after an upward shift, -1 after a downward one
    while True:
        iters += 1
        status = walk(build_table(cands, m), tail, ext, m, thr, p["max_walk_len"])
        if status == FORK and last >= 0 and m + p["shift"] <= p["max_mer_len"]:
            m += p["shift"]
            last = 1
        elif status == DEAD_END and last <= 0 and m - p["shift"] >= p["min_mer_len"]:
            m -= p["shift"]
            last = -1
        else:
            return ext, status, iters, m


def local_assm(contigs, reads, quals, alns, pairs, means=None, k=21, qual_offset=33, **params):
    """kc_local_assm: (block bytes, offsets uint64[n_ctgs + 1], ends LASSM_END_DTYPE[2 n_ctgs], stats dict)"""
    p = dict(DEFAULTS)
    p.update(params)
    check_params(p)
    if len(reads) & 1:
        raise BadArg("%d reads are no pairs" % len(reads))
    for r, s in enumerate(reads):
        if len(s) > MAX_READ_LEN:
            raise BadRead(r)
    check_records(alns, [len(c) for c in contigs], [len(s) for s in reads], len(reads))
    check_pairs(pairs, alns, len(reads))
    cands = candidates(contigs, reads, quals, alns, pairs, p, qual_offset)
    ends = np.zeros(2 * len(contigs), dtype=LASSM_END_DTYPE)
    st = {"ends": 2 * len(contigs), "status": [0] * 6, "cands_overhang": 0, "cands_mate": 0, "cand_bases": 0, "iterations": 0,
          "ext_bases": 0, "ctgs_extended": 0}
    block, offsets = [], [0]
    for u, ctg in enumerate(contigs):
        exts = []
        for side in (0, 1):
            e = 2 * u + side
            cs = cands[e]
            st["cands_mate"] += sum(1 for c in cs if c[2])
            st["cands_overhang"] += sum(1 for c in cs if not c[2])
            st["cand_bases"] += sum(len(c[0]) for c in cs)
            if not cs or len(cs) > p["max_cands"]:
                ext, status, iters, m = [], (NO_CANDS if not cs else TOO_MANY), 0, 0
            else:
                walk_ctg = codes_of(ctg) if side else revcomp_codes(codes_of(ctg), [HI] * len(ctg))[0]
                tail = walk_ctg[len(walk_ctg) - min(len(ctg), p["max_mer_len"]):]
                ext, status, iters, m = extend_end(tail, cs, k, 0 if means is None else int(means[u]), p)
            exts.append(ext)
            ends[e] = (len(cs), len(ext), 0, iters, m, status)
            st["status"][status] += 1
            st["iterations"] += iters
            st["ext_bases"] += len(ext)
        left = "".join("ACGT"[3 - c] for c in reversed(exts[0]))
        right = "".join("ACGT"[c] for c in exts[1])
        ends[2 * u]["out_pos"] = offsets[-1]
        ends[2 * u + 1]["out_pos"] = offsets[-1] + len(left) + len(ctg)
        block.append(left + ctg + right + "_")
        offsets.append(offsets[-1] + len(block[-1]))
        st["ctgs_extended"] += 1 if exts[0] or exts[1] else 0
    return "".join(block).encode(), np.array(offsets, dtype=np.uint64), ends, st


def mirror(contigs, reads_len, alns):
    """the same alignments on the reverse complements of the contigs: contig coordinates flip, the orientation flips, the
    read coordinates turn into the other orientation's (a record's rstart / rstop are in the oriented read R')"""
    out = alns.copy()
    for i in range(len(alns)):
        a = alns[i]
        if int(a["kind"]) == KIND_NONE:
            out[i]["orient"] = 1 - int(a["orient"])
            continue
        n, L = len(contigs[int(a["ctg"])]), reads_len[int(a["read"])]
        out[i]["cstart"], out[i]["cstop"] = n - int(a["cstop"]), n - int(a["cstart"])
        out[i]["rstart"], out[i]["rstop"] = L - int(a["rstop"]), L - int(a["rstart"])
        out[i]["orient"] = 1 - int(a["orient"])
    return out
