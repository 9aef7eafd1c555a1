"""Host model of kc_ctg_polish (csrc/kc_polish.hpp): the definitions of include/kcount_mi355_polish.h and DESIGN.md section 33
in plain Python, a loop over the records and a loop over the columns with no cleverness.  The reference holds no contig or
alignment code, so this file IS the definition the device is compared with, byte for byte; tests/test_polish_model.py checks
it against cases whose answer follows from the case alone.

Contigs and reads are Python strings, qualities a list of bytes objects beside the reads (or None), records a GAP_ALN_DTYPE
array."""
import numpy as np

import depth_model as D
from gap_model import GAP_ALN_DTYPE, KIND_NONE, contig_codes, oriented, read_codes  # noqa: F401

BEST_ONLY = 1
MAX_EDGE = D.MAX_EDGE
MAX_PERMILLE = 1000
MAX_QUAL = 255
CTG_DTYPE = np.dtype([("votes", "<u8"), ("placed", "<u4"), ("changed", "<u4"), ("filled", "<u4"), ("disputed", "<u4"), ("thin", "<u4"),
                      ("uncovered", "<u4")])
FIX_DTYPE = np.dtype([("pos", "<u4"), ("ctg", "<u4"), ("old", "u1"), ("new", "u1"), ("top", "<u2"), ("tot", "<u2"), ("pad", "<u2")])
RECORD_CLASSES = ("none", "filtered", "not_best", "unequal", "divergent", "placed")
COLUMN_CLASSES = ("uncovered", "thin", "disputed", "confirmed", "changed")
STATS = ("records",) + RECORD_CLASSES + ("votes", "columns") + COLUMN_CLASSES + ("filled", "sort_passes")
DEFAULTS = dict(min_score=0, min_len=0, edge_clip=0, max_mismatches=8, min_depth=3, min_permille=700, min_qual=0, best_only=False)

BadArg, BadRecord, BadRead = D.BadArg, D.BadRecord, D.BadRead


class TooManyFixes(ValueError):
    pass


def check_params(edge_clip, min_depth, min_permille, min_qual, flags):
    if edge_clip > MAX_EDGE or flags & ~BEST_ONLY:
        raise BadArg("edge_clip %d over %d or unknown flags 0x%x" % (edge_clip, MAX_EDGE, flags))
    if min_depth < 1:
        raise BadArg("min_depth is 0, at least 1")
    if min_permille > MAX_PERMILLE:
        raise BadArg("min_permille is %d, at most %d" % (min_permille, MAX_PERMILLE))
    if min_qual > MAX_QUAL:
        raise BadArg("min_qual is %d, at most %d" % (min_qual, MAX_QUAL))


def sort_passes(nbytes, n_alns):
    """radix passes of eight bits over the bits of nbytes (none without records)"""
    return (max(nbytes, 1).bit_length() + 7) // 8 if n_alns else 0


def classify(rec, i, rp, cc, best, min_score, min_len, max_mismatches):
    """the class of record i; rp: R' as codes, cc: the contig's codes, best: the reads' best records or None"""
    if int(rec["kind"]) == KIND_NONE:
        return "none"
    if not D.passes(rec, min_score, min_len):
        return "filtered"
    if best is not None and best[int(rec["read"])] != i:
        return "not_best"
    cstart, cstop, rstart, rstop = int(rec["cstart"]), int(rec["cstop"]), int(rec["rstart"]), int(rec["rstop"])
    if cstop - cstart != rstop - rstart:
        return "unequal"
    m = 0
    for j in range(cstop - cstart):
        r, c = rp[rstart + j], cc[cstart + j]
        if r < 4 and c < 4 and r != c:
            m += 1
    return "divergent" if m > max_mismatches else "placed"


def decide(c, cur, min_depth, min_permille):
    """a column's class and winner from its four counts and the code it holds"""
    tot = sum(c)
    if tot == 0:
        return "uncovered", None
    if tot < min_depth:
        return "thin", None
    top = max(c)
    w = c.index(top)
    second = max(c[b] for b in range(4) if b != w)
    if not (top > second and top * 1000 >= min_permille * tot):
        return "disputed", None
    return ("confirmed" if w == cur else "changed"), w


def polish(contigs, reads, alns, quals=None, min_score=0, min_len=0, edge_clip=0, max_mismatches=8, min_depth=3, min_permille=700, min_qual=0,
           best_only=False, qual_offset=33, fix_capacity=None):
    """kc_ctg_polish: (out bytes of the block, counts uint16[nbytes, 4], ctgs CTG_DTYPE[n_ctgs], fixes FIX_DTYPE[changed], stats).
    fix_capacity: TooManyFixes beyond it, as the call answers KC_ERR_CAPACITY"""
    flags = BEST_ONLY if best_only else 0
    check_params(edge_clip, min_depth, min_permille, min_qual, flags)
    for r, read in enumerate(reads):
        if len(read) > D.MAX_READ_LEN:
            raise BadRead(r)
    ctg_lens, read_lens = [len(c) for c in contigs], [len(r) for r in reads]
    D.check_records(alns, ctg_lens, read_lens, len(reads))
    best = D.best_records(alns, len(reads), min_score, min_len) if best_only else None
    offs = D.block_offsets(ctg_lens)
    nbytes = offs[-1]
    cnt = [[0, 0, 0, 0] for _ in range(nbytes)]
    st = dict.fromkeys(STATS, 0)
    st["records"], st["columns"], st["sort_passes"] = len(alns), nbytes - len(contigs), sort_passes(nbytes, len(alns))
    ctgs = np.zeros(len(contigs), dtype=CTG_DTYPE)
    ccodes = [contig_codes(c) for c in contigs]
    gate = quals is not None and min_qual > 0
    for i in range(len(alns)):
        rec = alns[i]
        read, u, orient = int(rec["read"]), int(rec["ctg"]), int(rec["orient"])
        rp = oriented(read_codes(reads[read]), orient)
        cls = classify(rec, i, rp, ccodes[u], best, min_score, min_len, max_mismatches)
        st[cls] += 1
        if cls != "placed":
            continue
        ctgs[u]["placed"] += 1
        cstart, cstop, rstart = int(rec["cstart"]), int(rec["cstop"]), int(rec["rstart"])
        span, L = cstop - cstart, len(reads[read])
        e_lo = edge_clip if cstart > 0 else 0
        e_hi = edge_clip if cstop < ctg_lens[u] else 0
        for j in range(e_lo, span - e_hi):
            r = rstart + j
            b = rp[r]
            if b >= 4:
                continue
            if gate:
                q = quals[read][r] if orient == 0 else quals[read][L - 1 - r]
                if q - qual_offset < min_qual:
                    continue
            cnt[offs[u] + cstart + j][b] += 1
    out = bytearray(("".join(c + "_" for c in contigs)).encode())
    fixes = []
    for u, ctg in enumerate(contigs):
        for j in range(len(ctg)):
            pos = offs[u] + j
            c = cnt[pos]
            cur = ccodes[u][j]
            cls, w = decide(c, cur, min_depth, min_permille)
            st[cls] += 1
            st["votes"] += sum(c)
            ctgs[u]["votes"] += sum(c)
            if cls != "confirmed":
                ctgs[u][cls] += 1
            if cls == "changed":
                if cur == 4:
                    st["filled"] += 1
                    ctgs[u]["filled"] += 1
                fixes.append((pos, u, out[pos], ord("ACGT"[w]), min(max(c), 65535), min(sum(c), 65535), 0))
                out[pos] = ord("ACGT"[w])
    assert st["records"] == sum(st[k] for k in RECORD_CLASSES) and st["columns"] == sum(st[k] for k in COLUMN_CLASSES)
    if fix_capacity is not None and len(fixes) > fix_capacity:
        raise TooManyFixes("%d fixes, room for %d" % (len(fixes), fix_capacity))
    counts = np.minimum(np.array(cnt, dtype=np.int64).reshape(nbytes, 4), 65535).astype(np.uint16)
    return bytes(out), counts, ctgs, np.array(fixes, dtype=FIX_DTYPE), st
