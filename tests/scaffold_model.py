"""Host model of kc_scaffold (include/kcount_mi355.h): the rules in plain Python, loops and dicts
only.  The reference holds no scaffolding, so this file is the definition the device must equal byte for byte.

scaffold(contigs, links, **params) -> (seqs, offsets, scaffolds, members, ctg_member, stats): the block as bytes, the
n_scaffolds + 1 offsets, SCAFFOLD_DTYPE and MEMBER_DTYPE records, every contig's index in members, and the statistics as
a dict.  contigs: the texts, upper-case A C G T N; links: LINK_DTYPE records as kc_ctg_links writes them."""
import numpy as np

LINK_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("splints", "<u4"), ("spans", "<u4"), ("splint_gap_min", "<i4"), ("splint_gap_max", "<i4"),
                       ("span_gap_min", "<i4"), ("span_gap_max", "<i4"), ("splint_gap_sum", "<i8"), ("span_gap_sum", "<i8")])
SCAFFOLD_DTYPE = np.dtype([("first_member", "<u4"), ("n_members", "<u4"), ("len", "<u4"), ("n_bases", "<u4"), ("overlap_bases", "<u4"),
                           ("flags", "<u4"), ("pad", "<u4", (2,))])
MEMBER_DTYPE = np.dtype([("ctg", "<u4"), ("join", "<i4"), ("out_pos", "<u4"), ("orient", "u1"), ("pad", "u1", (3,))])
SCAF_STATS = ("contigs", "records", "qualifying", "ends_best", "ends_ambiguous", "ends_not_mutual", "edges_chosen", "overlaps_checked",
              "overlaps_rejected", "edges_joined", "scaffolds", "singletons", "circular", "bases", "n_bases", "overlap_bases", "longest")
DEFAULTS = dict(min_splints=1, min_spans=2, max_second_permille=0, overlap_slack=0, flags=0)
MAX_SLACK = 64
MAX_OVERLAP = 65535
INSERT_MAX = 65535
CIRCULAR = 1
FIGURES = ("splints", "spans", "splint_gap_min", "splint_gap_max", "span_gap_min", "span_gap_max", "splint_gap_sum", "span_gap_sum")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


class BadArg(ValueError):
    pass


class Capacity(ValueError):
    pass


def params(**kw):
    return dict(DEFAULTS, **kw)


def revc(s):
    return "".join(COMP[c] for c in reversed(s))


def check_params(p):
    if p["min_splints"] < 1 or p["min_spans"] < 1:
        raise BadArg("kc_scaffold: min_splints %d, min_spans %d below 1" % (p["min_splints"], p["min_spans"]))
    if p["max_second_permille"] > 1000:
        raise BadArg("kc_scaffold: max_second_permille %d over 1000" % p["max_second_permille"])
    if p["overlap_slack"] > MAX_SLACK:
        raise BadArg("kc_scaffold: overlap_slack %d over %d" % (p["overlap_slack"], MAX_SLACK))
    if p["flags"]:
        raise BadArg("kc_scaffold: unknown flags 0x%x" % p["flags"])


def link(frm, to, splints=0, spans=0, gap=0, span_gap=None):
    """one directed record with every supporter at the same gap"""
    sg = gap if span_gap is None else span_gap
    return (frm, to, splints, spans, gap if splints else 0, gap if splints else 0, sg if spans else 0, sg if spans else 0, gap * splints,
            sg * spans)


def records(rows, both=True):
    """LINK_DTYPE records of link() rows: every row and its mirror, in key order"""
    out = []
    for r in rows:
        out.append(tuple(r))
        if both:
            out.append((r[1], r[0]) + tuple(r[2:]))
    out.sort(key=lambda r: (r[0], r[1]))
    return np.array(out, dtype=LINK_DTYPE) if out else np.zeros(0, dtype=LINK_DTYPE)


def kind_ok(c, lo, hi, s):
    if c == 0:
        return lo == 0 and hi == 0 and s == 0
    return -MAX_OVERLAP <= lo <= hi <= INSERT_MAX and c * lo <= s <= c * hi


def first_invalid(links, n_ctgs):
    """the lowest index of a record that breaks a rule, or None"""
    n = len(links)
    key = [(int(x["from"]) << 32) | int(x["to"]) for x in links]
    for i in range(n):
        x = links[i]
        f, t, sp, pn = int(x["from"]), int(x["to"]), int(x["splints"]), int(x["spans"])
        ok = f < 2 * n_ctgs and t < 2 * n_ctgs and (f >> 1) != (t >> 1) and sp + pn >= 1
        ok = ok and kind_ok(sp, int(x["splint_gap_min"]), int(x["splint_gap_max"]), int(x["splint_gap_sum"]))
        ok = ok and kind_ok(pn, int(x["span_gap_min"]), int(x["span_gap_max"]), int(x["span_gap_sum"]))
        ok = ok and (i == 0 or key[i] > key[i - 1])
        if ok:  # the mirror, by the device's binary search: the first record whose key is not below (to, from)
            want = (t << 32) | f
            lo, hi = 0, n
            while lo < hi:
                mid = lo + ((hi - lo) >> 1)
                if key[mid] < want:
                    lo = mid + 1
                else:
                    hi = mid
            ok = lo < n and key[lo] == want and all(int(links[lo][q]) == int(x[q]) for q in FIGURES)
        if not ok:
            return i
    return None


def floor_mean(s, c):
    return (2 * s + c) // (2 * c)  # Python's // is the floor


def gap_of(x):
    if int(x["splints"]) > 0:
        return floor_mean(int(x["splint_gap_sum"]), int(x["splints"]))
    return floor_mean(int(x["span_gap_sum"]), int(x["spans"]))


def node_text(contigs, v):
    return revc(contigs[v >> 1]) if v & 1 else contigs[v >> 1]


def verify(A, B, gap, slack):
    """the join of A followed by B at this gap, or None: the overlap the text does not show"""
    if gap >= 0:
        return gap
    o = -gap
    tries = [o]
    for d in range(1, slack + 1):
        tries += [o + d, o - d]
    for t in tries:
        if not 1 <= t < min(len(A), len(B)):
            continue
        if all(A[len(A) - t + i] == B[i] and B[i] in "ACGT" for i in range(t)):
            return -t
    return None


def scaffold(contigs, links, **kw):
    p = params(**kw)
    check_params(p)
    n = len(contigs)
    n_ends = 2 * n
    bad = first_invalid(links, n)
    if bad is not None:
        raise BadArg("kc_scaffold: record %d is invalid" % bad)
    st = dict.fromkeys(SCAF_STATS, 0)
    st["contigs"], st["records"] = n, len(links)
    # ---- choosing
    best, ambiguous = {}, {}
    rows = {}
    for x in links:
        rows.setdefault(int(x["from"]), []).append(x)
    for e in range(n_ends):
        q = [x for x in rows.get(e, []) if int(x["splints"]) >= p["min_splints"] or int(x["spans"]) >= p["min_spans"]]
        st["qualifying"] += len(q)
        if not q:
            continue
        q.sort(key=lambda x: (-(int(x["splints"]) + int(x["spans"])), -int(x["splints"]), int(x["to"])))
        best[e] = q[0]
        sup = int(q[0]["splints"]) + int(q[0]["spans"])
        ambiguous[e] = len(q) > 1 and (int(q[1]["splints"]) + int(q[1]["spans"])) * 1000 > sup * p["max_second_permille"]
    st["ends_best"] = len(best)
    st["ends_ambiguous"] = sum(1 for e in best if ambiguous[e])
    partner, join = {}, {}
    for e in sorted(best):
        f = int(best[e]["to"])
        mutual = f in best and int(best[f]["to"]) == e
        if not mutual:
            st["ends_not_mutual"] += 1
        if not mutual or ambiguous[e] or ambiguous[f] or e > f:
            continue
        st["edges_chosen"] += 1
        gap = gap_of(best[e])
        A, B = node_text(contigs, e ^ 1), node_text(contigs, f)  # the node left through e is e ^ 1, the node entered through f is f
        if gap < 0:
            st["overlaps_checked"] += 1
        j = verify(A, B, gap, p["overlap_slack"])
        if j is None:
            st["overlaps_rejected"] += 1
            continue
        st["edges_joined"] += 1
        partner[e], partner[f] = f, e
        join[e] = join[f] = j
    # ---- walking: next(v) is the partner of the end v is left through, v ^ 1
    nxt = {v: partner.get(v ^ 1) for v in range(n_ends)}
    has_pred = set(w for w in nxt.values() if w is not None)
    seen, circ_cut = set(), set()
    for v in range(n_ends):  # what a walk from a node without predecessor reaches lies on a path ...
        w = v if v not in has_pred else None
        while w is not None:
            seen.add(w)
            w = nxt[w]
    for v in range(n_ends):  # ... and the rest on cycles: cut in front of (u*, +), the twin cycle behind (u*, -)
        if v in seen:
            continue
        cycle, w = [], v
        while w not in seen:
            seen.add(w)
            cycle.append(w)
            w = nxt[w]
        u = min(x >> 1 for x in cycle)
        if 2 * u in cycle:
            for x in cycle:
                if nxt[x] == 2 * u:
                    nxt[x] = None
            circ_cut.add(2 * u)
        else:
            nxt[2 * u + 1] = None
    pred = {v: None for v in range(n_ends)}
    for v in range(n_ends):
        if nxt[v] is not None:
            pred[nxt[v]] = v
    heads = []
    for v in range(n_ends):
        if pred[v] is not None:
            continue
        tail = v
        while nxt[tail] is not None:
            tail = nxt[tail]
        # the twin path's head is tail ^ 1
        if (v >> 1) < (tail >> 1) or (v == tail and not v & 1):
            heads.append(v)
    heads.sort(key=lambda v: v >> 1)
    # ---- text and records
    text, offsets, scafs, members = [], [0], [], []
    ctg_member = [0] * n
    pos = 0
    for h in heads:
        first, start = len(members), pos
        nb = ob = 0
        v = h
        while v is not None:
            t = node_text(contigs, v)
            j = 0 if v == h else join[v]  # the edge v is entered through: its entry end is v
            if j >= 0:
                text.append("N" * j)
                pos += j
                nb += j
                out_pos = pos
                text.append(t)
                pos += len(t)
            else:
                out_pos = pos
                text.append(t[-j:])
                pos += len(t) + j
                ob += -j
            ctg_member[v >> 1] = len(members)
            members.append((v >> 1, j, out_pos, v & 1, (0, 0, 0)))
            v = nxt[v]
        ln = pos - start
        scafs.append((first, len(members) - first, ln, nb, ob, CIRCULAR if h in circ_cut else 0, (0, 0)))
        text.append("_")
        pos += 1
        offsets.append(pos)
        st["singletons"] += len(members) - first == 1
        st["circular"] += h in circ_cut
        st["n_bases"] += nb
        st["overlap_bases"] += ob
        st["longest"] = max(st["longest"], ln)
    if pos >= 1 << 31:
        raise Capacity("kc_scaffold: the scaffolds are %d bytes, a block holds fewer than 2^31" % pos)
    st["scaffolds"] = len(heads)
    st["bases"] = pos - len(heads)
    st = {k: int(v) for k, v in st.items()}
    return ("".join(text).encode(), np.array(offsets, dtype=np.uint64), np.array(scafs, dtype=SCAFFOLD_DTYPE) if scafs else np.zeros(0, SCAFFOLD_DTYPE),
            np.array(members, dtype=MEMBER_DTYPE) if members else np.zeros(0, MEMBER_DTYPE), np.array(ctg_member, dtype=np.uint32), st)


def strings(result):
    seqs, offsets = result[0].decode(), result[1]
    return [seqs[int(offsets[i]):int(offsets[i + 1]) - 1] for i in range(len(offsets) - 1)]
