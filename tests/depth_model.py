"""Host model of kc_aln_depths and kc_pair_inserts (csrc/kc_depth.hpp): the definitions of include/kcount_mi355.h and
DESIGN.md section 17 in plain Python, a loop over the records with no cleverness.  The reference holds no code for
either step, so this file IS the definition the device is compared with, byte for byte; tests/test_depth_model.py checks
it against cases whose answer follows from the case alone.

Contigs are given by their lengths only (the calls never read a base); reads by their lengths."""
import numpy as np

from gap_model import GAP_ALN_DTYPE, KIND_NONE  # noqa: F401  (the records are kc_align_gapped's)

MAX_READ_LEN = 1024
MAX_EDGE = 1024
INSERT_MAX = 65535
BEST_ONLY, PER_CONTIG = 1, 2
PAIR_NONE, PAIR_ONE, PAIR_DIFF_CTG, PAIR_SAME_ORIENT, PAIR_EVERTED, PAIR_TOO_LONG, PAIR_PROPER = range(7)
NO_ALN = 0xFFFFFFFF
CTG_DEPTH_DTYPE = np.dtype([("depth_sum", "<u8"), ("len", "<u4"), ("covered", "<u4"), ("min_depth", "<u4"), ("max_depth", "<u4"),
                            ("alns", "<u4"), ("mean", "<u4")])
PAIR_DTYPE = np.dtype([("aln0", "<u4"), ("aln1", "<u4"), ("insert", "<u4"), ("cls", "u1"), ("pad", "u1", (3,))])
DEPTH_STATS = ("records", "none", "filtered", "not_best", "clipped_away", "used", "bases_covered", "depth_sum", "saturated")


class BadArg(ValueError):
    pass


class BadRecord(ValueError):
    """an invalid record: .index is the lowest bad index"""
    def __init__(self, index):
        ValueError.__init__(self, "record %d" % index)
        self.index = index


class BadRead(ValueError):
    def __init__(self, index):
        ValueError.__init__(self, "read %d" % index)
        self.index = index


def valid(rec, ctg_lens, read_lens=None, nreads=None):
    """nreads: read < nreads is part of validity; read_lens: also rstop <= L(read)"""
    ctg, orient, kind = int(rec["ctg"]), int(rec["orient"]), int(rec["kind"])
    if not (ctg < len(ctg_lens) and orient <= 1 and kind <= 2):
        return False
    if kind != KIND_NONE:
        cstart, cstop, rstart, rstop = int(rec["cstart"]), int(rec["cstop"]), int(rec["rstart"]), int(rec["rstop"])
        if not (cstart < cstop <= ctg_lens[ctg] and rstart < rstop <= MAX_READ_LEN):
            return False
    if nreads is not None:
        if not int(rec["read"]) < nreads:
            return False
        if read_lens is not None and kind != KIND_NONE and not int(rec["rstop"]) <= read_lens[int(rec["read"])]:
            return False
    return True


def check_records(alns, ctg_lens, read_lens=None, nreads=None):
    for i in range(len(alns)):
        if not valid(alns[i], ctg_lens, read_lens, nreads):
            raise BadRecord(i)


def passes(rec, min_score, min_len):
    return int(rec["kind"]) != KIND_NONE and int(rec["score"]) >= min_score and int(rec["cstop"]) - int(rec["cstart"]) >= min_len


def best_records(alns, nreads, min_score, min_len):
    """every read's best record index, or None: the greatest score, the lowest index among equal scores"""
    best = [None] * nreads
    for i in range(len(alns)):
        if passes(alns[i], min_score, min_len):
            r = int(alns[i]["read"])
            if best[r] is None or int(alns[i]["score"]) > int(alns[best[r]]["score"]):
                best[r] = i
    return best


def block_offsets(ctg_lens):
    offs = [0]
    for n in ctg_lens:
        offs.append(offs[-1] + n + 1)
    return offs


def aln_depths(ctg_lens, alns, min_score=0, min_len=0, edge_clip=0, flags=0, nreads=0):
    """kc_aln_depths: (depths uint16[nbytes], ctgs CTG_DEPTH_DTYPE[n_ctgs], stats dict)"""
    if edge_clip > MAX_EDGE or flags & ~(BEST_ONLY | PER_CONTIG):
        raise BadArg("edge_clip %d over %d or unknown flags 0x%x" % (edge_clip, MAX_EDGE, flags))
    best_only = bool(flags & BEST_ONLY)
    check_records(alns, ctg_lens, None, nreads if best_only else None)
    best = best_records(alns, nreads, min_score, min_len) if best_only else None
    offs = block_offsets(ctg_lens)
    depth = [0] * offs[-1]
    st = dict.fromkeys(DEPTH_STATS, 0)
    st["records"] = len(alns)
    n_alns = [0] * len(ctg_lens)
    for i in range(len(alns)):
        rec = alns[i]
        if int(rec["kind"]) == KIND_NONE:
            st["none"] += 1
            continue
        if not passes(rec, min_score, min_len):
            st["filtered"] += 1
            continue
        if best_only and best[int(rec["read"])] != i:
            st["not_best"] += 1
            continue
        u, cstart, cstop = int(rec["ctg"]), int(rec["cstart"]), int(rec["cstop"])
        lo = cstart + (edge_clip if cstart > 0 else 0)
        hi = cstop - (edge_clip if cstop < ctg_lens[u] else 0)
        if lo >= hi:
            st["clipped_away"] += 1
            continue
        st["used"] += 1
        n_alns[u] += 1
        for j in range(lo, hi):
            depth[offs[u] + j] += 1
    ctgs = np.zeros(len(ctg_lens), dtype=CTG_DEPTH_DTYPE)
    out = np.zeros(offs[-1], dtype=np.uint16)
    for u, n in enumerate(ctg_lens):
        d = depth[offs[u]:offs[u] + n]
        mean = min(65535, (sum(d) + n // 2) // n) if n else 0
        ctgs[u] = (sum(d), n, sum(1 for x in d if x > 0), min(d) if n else 0, max(d) if n else 0, n_alns[u], mean)
        assert depth[offs[u] + n] == 0  # the separator
        for j in range(n):
            out[offs[u] + j] = mean if flags & PER_CONTIG else min(d[j], 65535)
    st["bases_covered"] = sum(1 for x in depth if x > 0)
    st["depth_sum"] = sum(depth)
    st["saturated"] = sum(1 for x in depth if x > 65535)
    assert st["records"] == st["none"] + st["filtered"] + st["not_best"] + st["clipped_away"] + st["used"]
    return out, ctgs, st


def classify(b0, b1, read_lens, max_insert):
    """(class, insert) of a pair from its mates' best records (None: no record)"""
    if b0 is None and b1 is None:
        return PAIR_NONE, 0
    if b0 is None or b1 is None:
        return PAIR_ONE, 0
    if int(b0["ctg"]) != int(b1["ctg"]):
        return PAIR_DIFF_CTG, 0
    if int(b0["orient"]) == int(b1["orient"]):
        return PAIR_SAME_ORIENT, 0
    F, R = (b0, b1) if int(b0["orient"]) == 0 else (b1, b0)
    fs = int(F["cstart"]) - int(F["rstart"])
    rs = int(R["cstart"]) - int(R["rstart"])
    re = int(R["cstop"]) + (read_lens[int(R["read"])] - int(R["rstop"]))
    if rs < fs:
        return PAIR_EVERTED, 0
    insert = re - fs
    assert insert >= 1
    return (PAIR_PROPER if insert <= max_insert else PAIR_TOO_LONG), insert


def pair_inserts(ctg_lens, read_lens, alns, max_insert=INSERT_MAX, min_score=0, min_len=0):
    """kc_pair_inserts: (hist uint64[max_insert + 1], pairs PAIR_DTYPE[nreads / 2], stats dict)"""
    if not 1 <= max_insert <= INSERT_MAX:
        raise BadArg("max_insert %d outside 1 .. %d" % (max_insert, INSERT_MAX))
    nreads = len(read_lens)
    if nreads & 1:
        raise BadArg("%d reads are no pairs" % nreads)
    for r, n in enumerate(read_lens):
        if n > MAX_READ_LEN:
            raise BadRead(r)
    check_records(alns, ctg_lens, read_lens, nreads)
    best = best_records(alns, nreads, min_score, min_len)
    hist = np.zeros(max_insert + 1, dtype=np.uint64)
    pairs = np.zeros(nreads // 2, dtype=PAIR_DTYPE)
    st = {"pairs": nreads // 2, "cls": [0] * 7, "insert_sum": 0, "insert_sq_sum": 0, "reads_with_best": sum(1 for b in best if b is not None)}
    for p in range(nreads // 2):
        i0, i1 = best[2 * p], best[2 * p + 1]
        cls, insert = classify(None if i0 is None else alns[i0], None if i1 is None else alns[i1], read_lens, max_insert)
        pairs[p] = (NO_ALN if i0 is None else i0, NO_ALN if i1 is None else i1, insert, cls, (0, 0, 0))
        st["cls"][cls] += 1
        if cls == PAIR_PROPER:
            hist[insert] += 1
            st["insert_sum"] += insert
            st["insert_sq_sum"] += insert * insert
    return hist, pairs, st


def rec(read, ctg, cstart, cstop, rstart=0, rstop=None, score=None, orient=0, kind=0, mismatches=0, seeds=1):
    """a kc_gap_aln as a tuple: rstop by default rstart + the contig interval's length (at most a read's 1024), score
    twice that length"""
    if rstop is None:
        rstop = min(rstart + (cstop - cstart), MAX_READ_LEN)
    if score is None:
        score = 2 * (cstop - cstart)
    return (read, ctg, cstart, cstop, rstart, rstop, score, mismatches, seeds, orient, kind, (0, 0))


def records(rows):
    return np.array(rows, dtype=GAP_ALN_DTYPE)
