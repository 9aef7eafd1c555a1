"""The rules of kc_ctg_break (include/kcount_mi355_break.h) restated in plain Python and numpy, statement
by statement.  The device equals this model byte for byte; the model itself is held to cases whose answer follows from the
case alone (tests/test_break_model.py).  All arithmetic is Python integers; the tracks are exact, saturated only on the way out."""
import numpy as np

NO_ALN = 0xFFFFFFFF
ONE_MATE = 1
INSERT_MAX = 65535
PIECE_DTYPE = np.dtype([("ctg", "<u4"), ("start", "<u4"), ("len", "<u4"), ("flags", "<u4")])
BREAK_DTYPE = np.dtype([("ctg", "<u4"), ("pos", "<u4"), ("run_start", "<u4"), ("run_len", "<u4"), ("span", "<u4"), ("disc", "<u4"), ("piece", "<u4"),
                        ("pad", "<u4")])
STATS = ("pairs", "spanning", "discordant_pairs", "one_mate", "none", "disc_mates", "empty_intervals", "span_sum", "disc_sum", "columns", "interior",
         "weak", "runs", "short_runs", "breaks", "broken_contigs", "pieces")
DEFAULTS = dict(max_insert=1000, max_span=0, min_disc=3, margin=None, min_run=1, one_mate=False)


def spanning(a0, a1, len0, len1, max_insert):
    """Both mates present.  The interval [fs, re) of a spanning pair, not yet clamped, or None: both mates are discordant.
    a0 / a1: the records; len0 / len1: their reads' lengths."""
    if int(a0["ctg"]) != int(a1["ctg"]) or int(a0["orient"]) == int(a1["orient"]):
        return None
    (F, _), (R, LR) = ((a0, len0), (a1, len1)) if int(a0["orient"]) == 0 else ((a1, len1), (a0, len0))
    fs = int(F["cstart"]) - int(F["rstart"])
    rs = int(R["cstart"]) - int(R["rstart"])
    re = int(R["cstop"]) + (LR - int(R["rstop"]))
    if rs >= fs and re - fs <= max_insert:
        return fs, re
    return None


def disc_interval(a, L, max_insert):
    """where a discordant mate's partner should have been found, not yet clamped"""
    if int(a["orient"]) == 0:
        s = int(a["cstart"]) - int(a["rstart"])
        return s, s + max_insert
    e = int(a["cstop"]) + (L - int(a["rstop"]))
    return e - max_insert, e


def tracks(lens, read_lens, alns, pairs, max_insert, one_mate):
    """(span, disc, stats): per contig the two exact tracks as int64 arrays, and the pair statistics"""
    dspan = [np.zeros(n + 1, dtype=np.int64) for n in lens]
    ddisc = [np.zeros(n + 1, dtype=np.int64) for n in lens]
    st = dict.fromkeys(STATS, 0)
    st["pairs"] = len(pairs)
    cols = {f: alns[f].tolist() for f in ("ctg", "cstart", "cstop", "rstart", "rstop", "orient")} if len(alns) else {}
    rec = lambda i: {f: v[i] for f, v in cols.items()}  # noqa: E731  record i as plain integers
    aln0, aln1 = pairs["aln0"].tolist() if len(pairs) else [], pairs["aln1"].tolist() if len(pairs) else []
    read_lens = [int(x) for x in read_lens]

    def add(diff, u, lo, hi):
        lo, hi = max(lo, 0), min(hi, lens[u])
        if lo >= hi:
            st["empty_intervals"] += 1
            return False
        diff[u][lo] += 1
        diff[u][hi] -= 1
        return True

    def discordant(i, read):
        a = rec(i)
        if add(ddisc, a["ctg"], *disc_interval(a, read_lens[read], max_insert)):
            st["disc_mates"] += 1

    for p in range(len(pairs)):
        i0, i1 = aln0[p], aln1[p]
        has0, has1 = i0 != NO_ALN, i1 != NO_ALN
        if has0 and has1:
            a0 = rec(i0)
            iv = spanning(a0, rec(i1), read_lens[2 * p], read_lens[2 * p + 1], max_insert)
            if iv is not None:
                st["spanning"] += 1
                add(dspan, a0["ctg"], *iv)
            else:
                st["discordant_pairs"] += 1
                discordant(i0, 2 * p)
                discordant(i1, 2 * p + 1)
        elif has0 or has1:
            st["one_mate"] += 1
            if one_mate:
                discordant(i0 if has0 else i1, 2 * p if has0 else 2 * p + 1)
        else:
            st["none"] += 1
    return [np.cumsum(d)[:-1] for d in dspan], [np.cumsum(d)[:-1] for d in ddisc], st


def runs_of(weak):
    """the maximal runs [a, b) of True in a boolean array"""
    w = np.concatenate(([False], weak, [False])).astype(np.int8)
    d = np.diff(w)
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def break_contigs(contigs, read_lens, alns, pairs, depths=None, max_insert=1000, max_span=0, min_disc=3, margin=None, min_run=1, one_mate=False):
    """contigs: a list of strings; read_lens: every read's length; alns / pairs: the records; depths: one value per byte of the
    input block or None.  Returns (block bytes, offsets, depths or None, pieces, breaks, stats, (span, disc) as uint16 over the
    input block)."""
    margin = max_insert if margin is None else margin
    assert 1 <= max_insert <= INSERT_MAX and margin >= 1 and min_run >= 1 and len(read_lens) == 2 * len(pairs)
    lens = [len(c) for c in contigs]
    span, disc, st = tracks(lens, read_lens, alns, pairs, max_insert, one_mate)
    starts = np.concatenate(([0], np.cumsum([n + 1 for n in lens]))).astype(np.int64)
    nbytes = int(starts[-1])
    out, offsets, dout, pieces, breaks = [], [0], [], [], []
    span16, disc16 = np.zeros(nbytes, dtype=np.uint16), np.zeros(nbytes, dtype=np.uint16)
    for u, text in enumerate(contigs):
        n, o = lens[u], int(starts[u])
        i = np.arange(n)
        interior = (i >= margin) & (i < n - margin)
        weak = interior & (span[u] <= max_span) & (disc[u] >= min_disc)
        span16[o:o + n] = np.minimum(span[u], 65535)
        disc16[o:o + n] = np.minimum(disc[u], 65535)
        st["columns"] += n
        st["interior"] += int(interior.sum())
        st["weak"] += int(weak.sum())
        st["span_sum"] += int(span[u].sum())
        st["disc_sum"] += int(disc[u].sum())
        cuts = []
        for a, b in runs_of(weak):
            st["runs"] += 1
            if b - a >= min_run:
                m = a + (b - a) // 2
                cuts.append(m)
                # the piece that begins at m: this contig's first piece, the cuts before m, and one
                breaks.append((u, m, a, b - a, int(span[u][m]), int(disc[u][m]), len(pieces) + len(cuts), 0))
            else:
                st["short_runs"] += 1
        st["breaks"] += len(cuts)
        st["broken_contigs"] += 1 if cuts else 0
        edges = [0] + cuts + [n]
        for k in range(len(edges) - 1):
            s, e = edges[k], edges[k + 1]
            pieces.append((u, s, e - s, (1 if k > 0 else 0) | (2 if k < len(edges) - 2 else 0)))
            out.append(text[s:e] + "_")
            offsets.append(offsets[-1] + e - s + 1)
            if depths is not None:
                dout.append(np.concatenate((np.asarray(depths[o + s:o + e], dtype=np.uint16), np.zeros(1, dtype=np.uint16))))
    st["pieces"] = len(pieces)
    assert st["pairs"] == st["spanning"] + st["discordant_pairs"] + st["one_mate"] + st["none"] and st["runs"] == st["short_runs"] + st["breaks"]
    d = None if depths is None else (np.concatenate(dout) if dout else np.zeros(0, dtype=np.uint16))
    return ("".join(out).encode(), np.array(offsets, dtype=np.uint64), d, np.array(pieces, dtype=PIECE_DTYPE).reshape(-1),
            np.array(breaks, dtype=BREAK_DTYPE).reshape(-1), st, (span16, disc16))
