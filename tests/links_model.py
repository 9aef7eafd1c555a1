"""Host model of kc_ctg_links (csrc/kc_links.hpp): the definitions of include/kcount_mi355.h and DESIGN.md section 19 in
plain Python, loops over the reads, their records and the pairs with no cleverness.  The reference holds no code for
this step, so this file IS the definition the device is compared with, byte for byte; tests/test_links_model.py checks
it against cases whose answer follows from the case alone.

Contigs are given by their lengths only (the call never reads a base); reads by their lengths."""
import numpy as np

from depth_model import INSERT_MAX, MAX_READ_LEN, NO_ALN, PAIR_DTYPE, BadArg, BadRead, BadRecord, check_records, passes  # noqa: F401
from gap_model import GAP_ALN_DTYPE, KIND_NONE  # noqa: F401
from lassm_model import BadPair, check_pairs  # noqa: F401

MAX_SLACK = 1024
MAX_OVERLAP = 65535
MAX_READ_ALNS = 64
LINK_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("splints", "<u4"), ("spans", "<u4"), ("splint_gap_min", "<i4"),
                       ("splint_gap_max", "<i4"), ("span_gap_min", "<i4"), ("span_gap_max", "<i4"), ("splint_gap_sum", "<i8"),
                       ("span_gap_sum", "<i8")])
LINK_STATS = ("reads", "reads_over_cap", "records", "none", "filtered", "passed", "splint_cands", "splints_gap_out", "span_cands",
              "spans_too_far", "links", "links_splint_only", "links_span_only", "links_both", "ends_linked")
DEFAULTS = dict(min_score=0, min_len=0, end_slack=5, max_overlap=200, max_splint_gap=100, insert_avg=300, max_insert=1000, max_read_alns=8,
                flags=0)


def params(**kw):
    p = dict(DEFAULTS, **kw)
    assert set(p) == set(DEFAULTS)
    return p


def check_params(p):
    if p["end_slack"] > MAX_SLACK:
        raise BadArg("end_slack %d over %d" % (p["end_slack"], MAX_SLACK))
    if p["max_overlap"] > MAX_OVERLAP or p["max_splint_gap"] > MAX_SLACK:
        raise BadArg("max_overlap %d over %d or max_splint_gap %d over %d" % (p["max_overlap"], MAX_OVERLAP, p["max_splint_gap"], MAX_SLACK))
    if not 1 <= p["insert_avg"] <= p["max_insert"] <= INSERT_MAX:
        raise BadArg("insert_avg %d, max_insert %d outside 1 <= insert_avg <= max_insert <= %d" % (p["insert_avg"], p["max_insert"], INSERT_MAX))
    if not 2 <= p["max_read_alns"] <= MAX_READ_ALNS:
        raise BadArg("max_read_alns %d outside 2 .. %d" % (p["max_read_alns"], MAX_READ_ALNS))
    if p["flags"]:
        raise BadArg("unknown flags 0x%x" % p["flags"])


def _rows(alns):
    """the records as dicts of plain integers"""
    cols = {n: alns[n].tolist() for n in ("read", "ctg", "cstart", "cstop", "rstart", "rstop", "score", "orient", "kind")}
    return [{n: cols[n][i] for n in cols} for i in range(len(alns))]


def leaves(a, len_u, slack):
    """(end, e) through which record a leaves its contig, or None"""
    if a["orient"] == 0:
        end, e = 2 * a["ctg"] + 1, len_u - a["cstop"]
    else:
        end, e = 2 * a["ctg"], a["cstart"]
    return (end, e) if e <= slack else None


def enters(a, len_u, slack):
    """(end, e) through which record a enters its contig, or None"""
    if a["orient"] == 0:
        end, e = 2 * a["ctg"], a["cstart"]
    else:
        end, e = 2 * a["ctg"] + 1, len_u - a["cstop"]
    return (end, e) if e <= slack else None


def interval(a, L):
    """[qs, qe) of the read, in the read's own direction"""
    return (a["rstart"], a["rstop"]) if a["orient"] == 0 else (L - a["rstop"], L - a["rstart"])


def points_out(b, len_u, L):
    """(end, d): where a mate with best record b points out of its contig, and how far that end is"""
    if b["orient"] == 0:
        return 2 * b["ctg"] + 1, len_u - (b["cstart"] - b["rstart"])
    return 2 * b["ctg"], b["cstop"] + (L - b["rstop"])


def candidates(ctg_lens, read_lens, alns, pairs, p, st):
    """[(end, end, kind, gap)], kind 0 a splint, 1 a span; counts into st"""
    rows = _rows(alns)
    by_read = [[] for _ in read_lens]
    for a in rows:
        if a["kind"] == KIND_NONE:
            st["none"] += 1
        elif not (a["score"] >= p["min_score"] and a["cstop"] - a["cstart"] >= p["min_len"]):
            st["filtered"] += 1
        else:
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
                    st["splint_cands"] += 1
                    out.append((lv[0], en[0], 0, gap))
                else:
                    st["splints_gap_out"] += 1
    if pairs is not None:
        for q in range(len(read_lens) // 2):
            i0, i1 = int(pairs[q]["aln0"]), int(pairs[q]["aln1"])
            if i0 == NO_ALN or i1 == NO_ALN or rows[i0]["ctg"] == rows[i1]["ctg"]:
                continue
            e0, d0 = points_out(rows[i0], ctg_lens[rows[i0]["ctg"]], read_lens[2 * q])
            e1, d1 = points_out(rows[i1], ctg_lens[rows[i1]["ctg"]], read_lens[2 * q + 1])
            if d0 + d1 <= p["max_insert"]:
                st["span_cands"] += 1
                out.append((e0, e1, 1, p["insert_avg"] - d0 - d1))
            else:
                st["spans_too_far"] += 1
    return out


def ctg_links(ctg_lens, read_lens, alns, pairs=None, **kw):
    """kc_ctg_links: (links LINK_DTYPE[n], end_first uint64[2 n_ctgs + 1], stats dict)"""
    p = params(**kw)
    check_params(p)
    nreads = len(read_lens)
    if nreads & 1:
        raise BadArg("%d reads are no pairs" % nreads)
    for r, n in enumerate(read_lens):
        if n > MAX_READ_LEN:
            raise BadRead(r)
    check_records(alns, ctg_lens, read_lens, nreads)
    if pairs is not None:
        check_pairs(pairs, alns, nreads)
    st = dict.fromkeys(LINK_STATS, 0)
    st["reads"], st["records"] = nreads, len(alns)
    links = {}  # (lo end, hi end) -> [splint gaps], [span gaps]
    for e0, e1, kind, gap in candidates(ctg_lens, read_lens, alns, pairs, p, st):
        links.setdefault((min(e0, e1), max(e0, e1)), ([], []))[kind].append(gap)
    assert st["records"] == st["none"] + st["filtered"] + st["passed"]
    directed = sorted([(lo, hi) for lo, hi in links] + [(hi, lo) for lo, hi in links])
    out = np.zeros(len(directed), dtype=LINK_DTYPE)
    for j, (f, t) in enumerate(directed):
        sp, sn = links[(min(f, t), max(f, t))]
        out[j] = (f, t, len(sp), len(sn), min(sp, default=0), max(sp, default=0), min(sn, default=0), max(sn, default=0), sum(sp), sum(sn))
    n_ends = 2 * len(ctg_lens)
    end_first = np.zeros(n_ends + 1, dtype=np.uint64)
    for f, _ in directed:  # end_first[e] = the records whose from is below e
        end_first[f + 1] += 1
    for e in range(n_ends):
        end_first[e + 1] += end_first[e]
    for sp, sn in links.values():
        st["links"] += 1
        st["links_both" if sp and sn else "links_splint_only" if sp else "links_span_only"] += 1
    st["ends_linked"] = len({f for f, _ in directed})
    return out, end_first, st


def mean_gap(links):
    """the wrapper's float column: the splint mean where there are splints, else the span mean"""
    out = np.zeros(len(links), dtype=np.float64)
    for j in range(len(links)):
        s, n = int(links[j]["splints"]), int(links[j]["spans"])
        out[j] = int(links[j]["splint_gap_sum"]) / s if s else int(links[j]["span_gap_sum"]) / n
    return out
