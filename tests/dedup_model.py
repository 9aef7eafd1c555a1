"""Host model of kc_ctg_dedup (include/kcount_mi355.h), written from the rules, statement by statement:
plain Python over byte strings, a dict of anchor texts in place of the device's table.  The device equals it byte for byte
(tests/test_gpu_ctg_dedup.py); tests/test_dedup_model.py holds the model itself to brute force and to Python's `in`."""
import numpy as np

DUPLICATES_ONLY = 1
KEPT, DUPLICATE, CONTAINED = range(3)
UNANCHORED = 1
NONE = 0xFFFFFFFF
DEFAULT_MAX_CANDIDATES = 1 << 26
# kc_dedup_stats in header order
STATS = ("contigs", "bases", "anchored", "unanchored", "windows", "window_hits", "candidates", "verified", "duplicates", "contained", "kept",
         "kept_bases", "removed_bases", "longest_removed")
REC_DTYPE = np.dtype([("status", "<u4"), ("container", "<u4"), ("pos", "<u4"), ("mismatches", "<u4"), ("new_index", "<u4"), ("len", "<u4"),
                      ("absorbed", "<u4"), ("orient", "u1"), ("flags", "u1"), ("pad", "u1", (2,))])
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = frozenset(b"ACGT")


class Capacity(Exception):
    pass


def rc(t):
    """the reverse complement, N staying N"""
    return t.translate(_COMP)[::-1]


def as_bytes(ctgs):
    return [c.encode() if isinstance(c, str) else bytes(c) for c in ctgs]


def block(ctgs, depths=None):
    """contigs -> (seqs, offsets[, depths per byte with 0 on the separators]) as kc_ctg_index_build takes them"""
    ctgs = as_bytes(ctgs)
    seqs = np.frombuffer(b"".join(c + b"_" for c in ctgs), dtype=np.uint8).copy()
    offsets = np.zeros(len(ctgs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) + 1 for c in ctgs])
    if depths is None:
        return seqs, offsets
    d = np.zeros(len(seqs), dtype=np.uint16)
    for u, c in enumerate(ctgs):
        d[int(offsets[u]):int(offsets[u]) + len(c)] = depths[u]
    return seqs, offsets, d


def split(seqs, offsets):
    text = bytes(np.asarray(seqs, dtype=np.uint8))
    return [text[int(offsets[i]):int(offsets[i + 1]) - 1] for i in range(len(offsets) - 1)]


def windows(t, k):
    """the positions w for which t[w, w + k) is all A C G T, in ascending order"""
    out, run = [], 0
    for i, c in enumerate(t):
        run = run + 1 if c in _ACGT else 0
        if run >= k:
            out.append(i + 1 - k)
    return out


def outranks(ctgs, v, u):
    return len(ctgs[v]) > len(ctgs[u]) or (len(ctgs[v]) == len(ctgs[u]) and v < u)


def mismatches(tu, tv, j, o):
    a = np.frombuffer(rc(tu) if o else tu, dtype=np.uint8)
    return int(np.count_nonzero(a != np.frombuffer(tv, dtype=np.uint8)[j:j + len(tu)]))


def dedup(ctgs, k, max_mismatches=0, duplicates_only=False, depths=None, max_candidates=0):
    """ctgs: the contigs' texts; depths: None or one array of uint16 per contig (a value per base).  Returns a dict: records
    (REC_DTYPE), ctgs (the kept texts), seqs / offsets (their block), depths (per byte of the block, or None), stats."""
    ctgs = as_bytes(ctgs)
    n = len(ctgs)
    anchor = []
    for t in ctgs:
        w = windows(t, k)
        anchor.append(w[0] if w else None)
    # anchor text -> [(u, 0)], its reverse complement -> [(u, 1)]: v's window text equals the one or the other
    by_text = {}
    for u, t in enumerate(ctgs):
        if anchor[u] is not None:
            a = t[anchor[u]:anchor[u] + k]
            by_text.setdefault(a, []).append((u, 0))
            by_text.setdefault(rc(a), []).append((u, 1))
    st = dict.fromkeys(STATS, 0)
    cands = [[] for _ in range(n)]  # per u: (v, j, o)
    for v, tv in enumerate(ctgs):
        for w in windows(tv, k):
            st["windows"] += 1
            hit = by_text.get(tv[w:w + k])
            if not hit:
                continue
            st["window_hits"] += 1
            for u, o in hit:
                if u == v or not outranks(ctgs, v, u):
                    continue
                lu = len(ctgs[u])
                j = w - anchor[u] if o == 0 else w - (lu - k - anchor[u])
                if j < 0 or j + lu > len(tv):
                    continue
                if duplicates_only and len(tv) != lu:
                    continue
                st["candidates"] += 1
                cands[u].append((v, j, o))
    limit = max_candidates or DEFAULT_MAX_CANDIDATES
    if st["candidates"] > limit:
        raise Capacity("kc_ctg_dedup: %d candidates, max_candidates is %d" % (st["candidates"], limit))
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["container"] = NONE
    kept = []
    for u, t in enumerate(ctgs):
        verified = []
        for v, j, o in cands[u]:
            mm = mismatches(t, ctgs[v], j, o)
            if mm <= max_mismatches:
                verified.append((-len(ctgs[v]), v, j, o, mm))  # the greatest v under the order, then the smallest j, then o
        st["verified"] += len(verified)
        r = recs[u]
        r["len"] = len(t)
        r["flags"] = UNANCHORED if anchor[u] is None else 0
        if verified:
            _, v, j, o, mm = min(verified)
            r["status"] = DUPLICATE if len(ctgs[v]) == len(t) else CONTAINED
            r["container"], r["pos"], r["orient"], r["mismatches"] = v, j, o, mm
            r["new_index"] = NONE
            recs["absorbed"][v] += 1
            st["duplicates" if r["status"] == DUPLICATE else "contained"] += 1
            st["removed_bases"] += len(t)
            st["longest_removed"] = max(st["longest_removed"], len(t))
        else:
            r["new_index"] = len(kept)
            kept.append(u)
    st["contigs"] = n
    st["bases"] = sum(len(t) for t in ctgs)
    st["anchored"] = sum(a is not None for a in anchor)
    st["unanchored"] = n - st["anchored"]
    st["kept"] = len(kept)
    st["kept_bases"] = sum(len(ctgs[u]) for u in kept)
    out = [ctgs[u] for u in kept]
    seqs, offsets = block(out)
    d = None
    if depths is not None:
        d = np.zeros(len(seqs), dtype=np.uint16)
        for i, u in enumerate(kept):
            d[int(offsets[i]):int(offsets[i]) + len(ctgs[u])] = depths[u]
    return dict(records=recs, ctgs=out, kept=kept, seqs=seqs, offsets=offsets, depths=d, stats=st)


def brute(ctgs, u, max_mismatches=0):
    """Is T_u or rc(T_u) within max_mismatches of a substring of some T_v that outranks u?  Every position, no anchors."""
    ctgs = as_bytes(ctgs)
    t = ctgs[u]
    for v, tv in enumerate(ctgs):
        if v == u or not outranks(ctgs, v, u):
            continue
        for o in (0, 1):
            for j in range(len(tv) - len(t) + 1):
                if mismatches(t, tv, j, o) <= max_mismatches:
                    return True
    return False
