"""Host model of kc_close_gaps (include/kcount_mi355.h): the rules in plain Python, loops and dicts
only.  The reference holds no gap closing, so this file is the definition the device must equal byte for byte;
tests/test_close_model.py checks it against cases whose answer follows from the case alone.

close_gaps(contigs, reads, alns, scaffolds, members, **params) -> (seqs, offsets, scaffolds, members, closures, stats):
the block as bytes, the n_scaffolds + 1 offsets, SCAFFOLD_DTYPE, MEMBER_DTYPE and CLOSURE_DTYPE records and the statistics
as a dict.  contigs: the texts, upper-case A C G T N; reads: the texts as str or bytes, any byte."""
import numpy as np

from depth_model import MAX_READ_LEN, BadArg, BadRead, check_records
from gap_model import KIND_NONE
from links_model import MAX_OVERLAP, MAX_READ_ALNS, MAX_SLACK, _rows, enters, interval, leaves
from scaffold_model import INSERT_MAX, MEMBER_DTYPE, SCAFFOLD_DTYPE, Capacity, node_text

CLOSURE_DTYPE = np.dtype([("cands", "<u4"), ("reads", "<u4"), ("old_join", "<i4"), ("new_join", "<i4"), ("fill_pos", "<u4"), ("disputed", "<u4"),
                          ("status", "u1"), ("pad", "u1", (3,)), ("reserved", "<u4")])
HEAD, NOT_A_GAP, NO_READS, WEAK, FILLED, ABUT, OVERLAP, OVERLAP_REJECTED = range(8)
CLOSE_STATS = ("members", "joins", "gaps", "reads_over_cap", "passed", "cands", "cands_off_join", "gaps_no_reads", "gaps_weak", "filled",
               "abutted", "overlapped", "overlaps_rejected", "fill_bases", "n_bases_left", "disputed_cols")
DEFAULTS = dict(min_score=0, min_len=0, end_slack=5, max_overlap=200, max_splint_gap=100, min_reads=2, min_agree_permille=500, max_read_alns=8,
                flags=0)
COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


class BadScaffold(ValueError):
    """an invalid scaffold record: .index is the lowest bad index"""
    def __init__(self, index):
        ValueError.__init__(self, "scaffold %d" % index)
        self.index = index


class BadMember(ValueError):
    def __init__(self, index):
        ValueError.__init__(self, "member %d" % index)
        self.index = index


def params(**kw):
    p = dict(DEFAULTS, **kw)
    assert set(p) == set(DEFAULTS)
    return p


def check_params(p):
    if p["end_slack"] > MAX_SLACK:
        raise BadArg("kc_close_gaps: end_slack %d over %d" % (p["end_slack"], MAX_SLACK))
    if p["max_overlap"] > MAX_OVERLAP or p["max_splint_gap"] > MAX_SLACK:
        raise BadArg("kc_close_gaps: max_overlap %d over %d or max_splint_gap %d over %d"
                     % (p["max_overlap"], MAX_OVERLAP, p["max_splint_gap"], MAX_SLACK))
    if p["min_reads"] < 1:
        raise BadArg("kc_close_gaps: min_reads %d below 1" % p["min_reads"])
    if p["min_agree_permille"] > 1000:
        raise BadArg("kc_close_gaps: min_agree_permille %d over 1000" % p["min_agree_permille"])
    if not 2 <= p["max_read_alns"] <= MAX_READ_ALNS:
        raise BadArg("kc_close_gaps: max_read_alns %d outside 2 .. %d" % (p["max_read_alns"], MAX_READ_ALNS))
    if p["flags"]:
        raise BadArg("kc_close_gaps: unknown flags 0x%x" % p["flags"])


def check_scaffolds(scaffolds, n):
    """the heads' member indices; raises at the lowest bad scaffold"""
    if n and len(scaffolds) == 0:
        raise BadScaffold(0)
    at, heads = 0, set()
    for s in range(len(scaffolds)):
        first, cnt = int(scaffolds[s]["first_member"]), int(scaffolds[s]["n_members"])
        if s:  # against its predecessor's record as it stands
            at = int(scaffolds[s - 1]["first_member"]) + int(scaffolds[s - 1]["n_members"])
        ok = cnt >= 1 and first == at and first + cnt <= n and (s + 1 < len(scaffolds) or first + cnt == n)
        if not ok:
            raise BadScaffold(s)
        heads.add(first)
    return heads


def check_members(members, heads, ctg_lens):
    n = len(ctg_lens)
    owner = {}
    for m in range(n):
        u = int(members[m]["ctg"])
        if u < n and u not in owner:
            owner[u] = m
    for m in range(n):
        x = members[m]
        u, j = int(x["ctg"]), int(x["join"])
        ok = u < n and int(x["orient"]) <= 1 and not any(int(b) for b in x["pad"]) and owner[u] == m
        if ok and m in heads:
            ok = j == 0
        elif ok:
            ok = -MAX_OVERLAP <= j <= INSERT_MAX
            pu = int(members[m - 1]["ctg"])
            if ok and j < 0 and pu < n:  # a bad predecessor is the lower index anyway
                ok = -j < min(ctg_lens[pu], ctg_lens[u])
        if not ok:
            raise BadMember(m)


def splints(ctg_lens, read_lens, alns, p, st):
    """[(read, X, Y, gap, segment start, segment stop)] of every splint candidate, as links_model.candidates forms them"""
    by_read = [[] for _ in read_lens]
    for a in _rows(alns):
        if a["kind"] != KIND_NONE and a["score"] >= p["min_score"] and a["cstop"] - a["cstart"] >= p["min_len"]:
            st["passed"] += 1
            by_read[a["read"]].append(a)
    out = []
    for r, recs in enumerate(by_read):
        if len(recs) > p["max_read_alns"]:
            st["reads_over_cap"] += 1
            continue
        for a in recs:
            for b in recs:
                qs_a, qe_a = interval(a, read_lens[r])
                qs_b, qe_b = interval(b, read_lens[r])
                lv, en = leaves(a, ctg_lens[a["ctg"]], p["end_slack"]), enters(b, ctg_lens[b["ctg"]], p["end_slack"])
                if a["ctg"] == b["ctg"] or not (qs_a < qs_b and qe_a < qe_b) or lv is None or en is None:
                    continue
                gap = (qs_b - qe_a) - lv[1] - en[1]
                if -p["max_overlap"] <= gap <= p["max_splint_gap"]:
                    out.append((r, lv[0], en[0], gap, qe_a + lv[1], qs_b - en[1]))
    return out


def vote_code(byte):
    """0..3 for A C G T in either case, None for every other byte"""
    return {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}.get(byte)


def consensus(segments):
    """(fill, disputed columns) of segments of one length: [(bytes, backward)]"""
    g = len(segments[0][0])
    fill, disputed = bytearray(), 0
    for c in range(g):
        n = [0, 0, 0, 0]
        for text, backward in segments:
            code = vote_code(text[g - 1 - c] if backward else text[c])
            if code is not None:
                n[3 - code if backward else code] += 1
        best = max(n)
        fill.append(ord("ACGT"[n.index(best)]) if best else ord("N"))
        disputed += sum(1 for v in n if v) > 1
    return bytes(fill), disputed


def close_gaps(contigs, reads, alns, scaffolds, members, **kw):
    p = params(**kw)
    check_params(p)
    reads = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    n = len(contigs)
    ctg_lens, read_lens = [len(c) for c in contigs], [len(r) for r in reads]
    for r, L in enumerate(read_lens):
        if L > MAX_READ_LEN:
            raise BadRead(r)
    check_records(alns, ctg_lens, read_lens, len(reads))
    heads = check_scaffolds(scaffolds, n)
    check_members(members, heads, ctg_lens)
    st = dict.fromkeys(CLOSE_STATS, 0)
    st["members"], st["joins"] = n, n - len(scaffolds)
    node = [2 * int(x["ctg"]) + int(x["orient"]) for x in members]
    # ---- the gap joins' ends, and their candidates
    join_of = {}
    for m in range(n):
        if m not in heads and int(members[m]["join"]) > 0:
            join_of[(node[m - 1] ^ 1, node[m])] = (m, False)
            join_of[(node[m], node[m - 1] ^ 1)] = (m, True)
    cands = {}
    for r, X, Y, gap, s0, s1 in splints(ctg_lens, read_lens, alns, p, st):
        st["cands"] += 1
        if (X, Y) not in join_of:
            st["cands_off_join"] += 1
            continue
        m, backward = join_of[(X, Y)]
        cands.setdefault(m, []).append((gap, reads[r][s0:s1] if gap > 0 else b"", backward))
    # ---- a decision a member
    new_join, status, fills = [0] * n, [HEAD] * n, {}
    votes, disputed = [0] * n, [0] * n
    for m in range(n):
        old = int(members[m]["join"])
        new_join[m] = old
        if m in heads:
            continue
        if old <= 0:
            status[m] = NOT_A_GAP
            continue
        st["gaps"] += 1
        mine = cands.get(m, [])
        if not mine:
            status[m] = NO_READS
            continue
        count = {}
        for gap, _, _ in mine:
            count[gap] = count.get(gap, 0) + 1
        g, v = min(count.items(), key=lambda kv: (-kv[1], kv[0]))
        if not (v >= p["min_reads"] and v * 1000 >= len(mine) * p["min_agree_permille"]):
            status[m] = WEAK
            continue
        votes[m] = v
        if g > 0:
            status[m], new_join[m] = FILLED, g
            fills[m], disputed[m] = consensus([(text, backward) for gap, text, backward in mine if gap == g])
        elif g == 0:
            status[m], new_join[m] = ABUT, 0
        else:
            A, B, o = node_text(contigs, node[m - 1]), node_text(contigs, node[m]), -g
            if 1 <= o < min(len(A), len(B)) and all(A[len(A) - o + i] == B[i] and B[i] in "ACGT" for i in range(o)):
                status[m], new_join[m] = OVERLAP, g
            else:
                status[m] = OVERLAP_REJECTED
    for key, code in (("gaps_no_reads", NO_READS), ("gaps_weak", WEAK), ("filled", FILLED), ("abutted", ABUT), ("overlapped", OVERLAP),
                      ("overlaps_rejected", OVERLAP_REJECTED)):
        st[key] = status.count(code)
    # ---- text and records
    text, offsets, scafs_out = [], [0], []
    members_out, closures = np.zeros(n, MEMBER_DTYPE), np.zeros(n, CLOSURE_DTYPE)
    pos = 0
    for s in range(len(scaffolds)):
        first, cnt = int(scaffolds[s]["first_member"]), int(scaffolds[s]["n_members"])
        start, nb, ob = pos, 0, 0
        for m in range(first, first + cnt):
            t, j = node_text(contigs, node[m]).encode(), new_join[m]
            fill_pos = pos
            if j >= 0:
                if status[m] == FILLED:
                    text.append(fills[m])
                    st["fill_bases"] += j
                else:
                    text.append(b"N" * j)
                    nb += j
                pos += j
                out_pos = pos
                text.append(t)
                pos += len(t)
            else:
                out_pos = pos
                text.append(t[-j:])
                pos += len(t) + j
                ob += -j
            members_out[m] = (int(members[m]["ctg"]), j, out_pos, int(members[m]["orient"]), (0, 0, 0))
            closures[m] = (len(cands.get(m, [])), votes[m], int(members[m]["join"]), j, fill_pos, disputed[m], status[m], (0, 0, 0), 0)
        scafs_out.append((first, cnt, pos - start, nb, ob, int(scaffolds[s]["flags"]), (0, 0)))
        text.append(b"_")
        pos += 1
        offsets.append(pos)
        st["n_bases_left"] += nb
    st["disputed_cols"] = sum(disputed)
    if pos >= 1 << 31:
        raise Capacity("kc_close_gaps: the scaffolds are %d bytes, a block holds fewer than 2^31" % pos)
    st = {k: int(v) for k, v in st.items()}
    return (b"".join(text), np.array(offsets, dtype=np.uint64), np.array(scafs_out, dtype=SCAFFOLD_DTYPE) if scafs_out else np.zeros(0, SCAFFOLD_DTYPE),
            members_out, closures, st)


def strings(result):
    seqs, offsets = result[0].decode(), result[1]
    return [seqs[int(offsets[i]):int(offsets[i + 1]) - 1] for i in range(len(offsets) - 1)]
