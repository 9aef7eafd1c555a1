"""Host model of kc_align_gapped: the step around the dynamic programme in plain Python, statement
by statement; the dynamic programme itself is tests/trim_model.py::ssw_align, the restatement of the reference's
Aligner::Align(report_cigar = false) that tests/golden/ssw_ref_alignments.json (adapter-sized inputs) and
tests/golden/gap_ref_alignments.json (read-sized inputs, the cases of gap_ssw_cases below) pin against src/ssw compiled
unmodified.  Nothing here is shaped after the kernels.

Contigs and reads are str as in tests/align_model.py; records are ALN_DTYPE arrays as align_model.align_reads returns
them."""
import numpy as np

import align_model as A
import trim_model as T

MAX_PAD = 1024
KIND_EXACT, KIND_DP, KIND_NONE = 0, 1, 2
SCORES_ALTERNATE = (1, 1, 1, 1, 1)  # ALTERNATE_ALN_SCORES 11111: match, mismatch, gap open, gap extend, ambiguity
SCORES_BLASTN = (2, 3, 5, 2, 1)     # BLASTN_ALN_SCORES 23521, CMakeDefinitions.txt:133
SCORES_13521 = (1, 3, 5, 2, 1)
SCORE_SETS = {"11111": SCORES_ALTERNATE, "23521": SCORES_BLASTN, "13521": SCORES_13521}
GAP_ALN_DTYPE = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("cstart", "<u4"), ("cstop", "<u4"), ("rstart", "<u2"), ("rstop", "<u2"),
                          ("score", "<u4"), ("mismatches", "<u2"), ("seeds", "<u2"), ("orient", "u1"), ("kind", "u1"), ("pad", "u1", (2,))])
GAP_STATS = ("records", "exact", "dp", "none", "cells", "score_sum")


class BadArg(ValueError):
    pass


class BadRecord(ValueError):
    """an invalid record: .index is the lowest bad index"""
    def __init__(self, index):
        super().__init__("record %d" % index)
        self.index = index


def check_args(pad, scores, flags=0):
    match, mismatch, go, ge, amb = scores
    if not (1 <= match <= 9 and 0 <= mismatch <= 9 and 0 <= amb <= 9 and 1 <= ge <= go <= 9):
        raise BadArg("scores")
    if not 0 <= pad <= MAX_PAD:
        raise BadArg("pad")
    if flags & ~1:
        raise BadArg("flags")


def read_codes(read):
    """A C G T in either case are 0..3, anything else is 4 (U too: kc_align_reads' alphabet, not kBaseTranslation's)"""
    return ["ACGT".index(ch.upper()) if ch in "ACGTacgt" else 4 for ch in read]


def contig_codes(ctg):
    return ["ACGT".index(ch) if ch in "ACGT" else 4 for ch in ctg]


def oriented(codes, orient):
    """R': the read, or its reverse complement (a code c < 4 becomes 3 - c, 4 stays 4)"""
    return codes if orient == 0 else [3 - c if c < 4 else 4 for c in reversed(codes)]


def as_text(codes):
    return "".join("ACGTN"[c] for c in codes).encode()


def valid(rec, reads, contigs):
    read, ctg, orient = int(rec["read"]), int(rec["ctg"]), int(rec["orient"])
    if not (read < len(reads) and ctg < len(contigs) and orient <= 1):
        return False
    L, len_u = len(reads[read]), len(contigs[ctg])
    cstart, cstop, rstart, rstop = int(rec["cstart"]), int(rec["cstop"]), int(rec["rstart"]), int(rec["rstop"])
    d = cstart - rstart
    return (cstart < cstop <= len_u and rstart < rstop <= L and cstop - cstart == rstop - rstart
            and cstart == max(0, d) and cstop == min(len_u, d + L))


def gap_one(rp, cc, d, rstart, rstop, pad, scores, always_dp):
    """One valid record: R' and the contig as codes.  (cstart, cstop, rstart, rstop, score, mismatches, kind, cells)"""
    L, len_u = len(rp), len(cc)
    mismatches = 0
    for i in range(rstart, rstop):
        if rp[i] == 4 or cc[d + i] == 4 or rp[i] != cc[d + i]:
            mismatches += 1
    if mismatches == 0 and not always_dp:
        return d + rstart, d + rstop, rstart, rstop, scores[0] * (rstop - rstart), 0, KIND_EXACT, 0
    wlo, whi = max(0, d - pad), min(len_u, d + L + pad)
    a = T.ssw_align(as_text(rp), as_text(cc[wlo:whi]), scores)
    cells = L * (whi - wlo)
    if a["sw_score"] > 0:
        return (wlo + a["ref_begin"], wlo + a["ref_end"] + 1, a["query_begin"], a["query_end"] + 1, a["sw_score"], mismatches, KIND_DP,
                cells)
    return 0, 0, 0, 0, 0, mismatches, KIND_NONE, cells


def align_gapped(contigs, reads, alns, pad=16, scores=SCORES_BLASTN, always_dp=False):
    """kc_align_gapped: (records as a GAP_ALN_DTYPE array, stats dict).  BadArg / BadRecord where the call answers
    KC_ERR_INVALID_ARG.  A record's answer is a pure function of (read text, contig, orient, interval), so equal ones are
    computed once."""
    check_args(pad, scores)
    for r, read in enumerate(reads):
        if len(read) > A.MAX_READ_LEN:
            raise BadArg("read %d" % r)
    for i, rec in enumerate(alns):
        if not valid(rec, reads, contigs):
            raise BadRecord(i)
    out = np.zeros(len(alns), dtype=GAP_ALN_DTYPE)
    st = dict.fromkeys(GAP_STATS, 0)
    st["records"] = len(alns)
    done, rcodes, ccodes = {}, {}, {}
    for i, rec in enumerate(alns):
        read, ctg, orient = int(rec["read"]), int(rec["ctg"]), int(rec["orient"])
        cstart, rstart, rstop = int(rec["cstart"]), int(rec["rstart"]), int(rec["rstop"])
        key = (reads[read], ctg, orient, cstart, rstart, rstop)
        if key not in done:
            if reads[read] not in rcodes:
                rcodes[reads[read]] = read_codes(reads[read])
            if ctg not in ccodes:
                ccodes[ctg] = contig_codes(contigs[ctg])
            done[key] = gap_one(oriented(rcodes[reads[read]], orient), ccodes[ctg], cstart - rstart, rstart, rstop, pad, scores, always_dp)
        cs, ce, rs, re, score, mism, kind, cells = done[key]
        out[i] = (read, ctg, cs, ce, rs, re, score, mism, int(rec["seeds"]), orient, kind, (0, 0))
        st[("exact", "dp", "none")[kind]] += 1
        st["cells"] += cells
        st["score_sum"] += score
    return out, st


# ---- the seeded inputs of tests/golden/gap_ref_alignments.json -------------------------------------------------------
GAP_SEED = 20261018
NAMED_LENGTHS = (1, 2, 20, 63, 64, 65, 150, 191, 192, 193, 250, 300, 511, 512, 513, 1023, 1024)
PADS = (0, 1, 16, 64)
UNITS = ("A", "C", "G", "T", "AC", "AG", "CT", "GT", "AT", "CG", "ACG", "AAC", "ACT")


def _rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _place(rng, n):
    """a position of a sequence of n: within 3 bases of either end half of the time"""
    if n <= 1:
        return 0
    mode = int(rng.integers(0, 4))
    if mode == 0:
        return int(rng.integers(0, min(4, n)))
    if mode == 1:
        return int(rng.integers(max(0, n - 4), n))
    return int(rng.integers(0, n))


def _plant(rng, s, nsub, nindel):
    """nsub substitutions and nindel insertions or deletions of 1 to 3 bases"""
    s = list(s)
    for _ in range(nsub):
        if s:
            p = _place(rng, len(s))
            s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    for _ in range(nindel):
        p = _place(rng, len(s))
        ln = int(rng.integers(1, 4))
        if rng.integers(0, 2) or len(s) <= ln:
            s[p:p] = list(_rand_seq(rng, ln))
        else:
            del s[p:p + ln]
    return "".join(s)


def _decorate(rng, s):
    """an N or two, or a lower-case stretch, in one case of three"""
    s = list(s)
    mode = int(rng.integers(0, 6))
    if mode == 0 and s:
        for _ in range(int(rng.integers(1, 3))):
            s[int(rng.integers(0, len(s)))] = "Nn"[int(rng.integers(0, 2))]
    elif mode == 1 and s:
        a = int(rng.integers(0, len(s)))
        b = int(rng.integers(a, len(s) + 1))
        s[a:b] = [c.lower() for c in s[a:b]]
    return "".join(s)


def _window_case(rng, template, pad, nsub, nindel, clip, decorate=True, max_len=A.MAX_READ_LEN):
    """(read, window): the template with planted errors against the template inside `pad` random bases on either side;
    clip 1 / 2: the window loses its left / right padding and a few bases of the template, as at a contig's end"""
    read = _plant(rng, template, nsub, nindel)[:max_len]
    if not read:
        read = template[:1]
    left, right = _rand_seq(rng, pad), _rand_seq(rng, pad)
    body = template
    if clip == 1:
        left, body = "", body[int(rng.integers(0, min(len(body), 40))):]
    elif clip == 2:
        right, body = "", body[:len(body) - int(rng.integers(0, min(len(body), 40)))]
    window = left + body + right
    if not window:
        window = template[:1]
    if decorate:
        read, window = _decorate(rng, read), _decorate(rng, window)
    return read, window


# With equal gap open and extend penalties the reference's word lanes stop their lazy-F loop after one row
# (csrc/kc_trim.hpp); its answers then differ from the exact integers.  Word lanes need a score of 254, so the reads of
# the 11111 set stay below 254 bases by construction.
CAP_11111 = 253


def gap_ssw_cases(name):
    """The (query, reference) texts of one score set: reads against contig windows."""
    rng = np.random.default_rng(GAP_SEED + sorted(SCORE_SETS).index(name))
    cap = CAP_11111 if name == "11111" else A.MAX_READ_LEN
    out = []
    for q, r in _gap_ssw_cases(rng, cap):
        assert 1 <= len(q) <= cap and r
        out.append((q, r))
    return out


def _gap_ssw_cases(rng, cap):
    out = []
    # every named length at every pad: one indel in the middle; errors towards the ends; a clipped window
    for L in NAMED_LENGTHS:
        L = min(L, cap)
        for pad in PADS:
            ln = int(rng.integers(1, 4))  # a read of exactly L bases
            if L > 2 * ln + 2 and rng.integers(0, 2):
                t = _rand_seq(rng, L + ln)
                read = t[:L // 2] + t[L // 2 + ln:]
            elif L > ln:
                t = _rand_seq(rng, L - ln)
                read = t[:(L - ln) // 2] + _rand_seq(rng, ln) + t[(L - ln) // 2:]
            else:
                t = read = _rand_seq(rng, L)
            out.append((read, _rand_seq(rng, pad) + t + _rand_seq(rng, pad)))
            out.append(_window_case(rng, _rand_seq(rng, L), pad, int(rng.integers(0, 6)), int(rng.integers(0, 4)), 0, max_len=cap))
            out.append(_window_case(rng, _rand_seq(rng, L), pad, int(rng.integers(0, 3)), int(rng.integers(0, 2)), 1 + int(rng.integers(0, 2)),
                                    max_len=cap))
    # a spread of lengths between those
    for rep in range(640):
        L = min(int(rng.integers(3, 330)), cap)
        clip = int(rng.integers(0, 3)) if rep % 4 == 0 else 0
        out.append(_window_case(rng, _rand_seq(rng, L), PADS[int(rng.integers(0, 4))], int(rng.integers(0, 6)), int(rng.integers(0, 4)), clip,
                                max_len=cap))
    for rep in range(60):
        L = min(int(rng.integers(330, 1025)), cap)
        out.append(_window_case(rng, _rand_seq(rng, L), PADS[int(rng.integers(0, 4))], int(rng.integers(0, 6)), int(rng.integers(0, 4)),
                                int(rng.integers(0, 3)) if rep % 4 == 0 else 0, max_len=cap))
    # homopolymer, di- and trinucleotide contigs: the tie rules
    for rep in range(420):
        unit = UNITS[int(rng.integers(0, len(UNITS)))]
        L = min(int(rng.integers(4, 200)) if rep % 10 else int(rng.integers(200, 600)), cap)
        t = (unit * 700)[int(rng.integers(0, 3)):][:L]
        pad = PADS[int(rng.integers(0, 4))]
        read = _plant(rng, t, int(rng.integers(0, 3)), int(rng.integers(0, 3)))[:cap] or t[:1]
        if rep % 3 == 0:
            window = _rand_seq(rng, pad) + t + _rand_seq(rng, pad)
        else:
            window = (unit * 700)[int(rng.integers(0, 3)):][:L + 2 * pad]
        out.append((_decorate(rng, read), _decorate(rng, window)))
    # a read that is half random
    for rep in range(120):
        L = min(int(rng.integers(20, 330)), cap)
        t = _rand_seq(rng, L)
        half = L // 2
        read = t[:half] + _rand_seq(rng, L - half) if rep % 2 else _rand_seq(rng, half) + t[half:]
        pad = PADS[int(rng.integers(0, 4))]
        out.append((_plant(rng, read, int(rng.integers(0, 3)), int(rng.integers(0, 2)))[:cap],
                    _rand_seq(rng, pad) + t + _rand_seq(rng, pad)))
    # unrelated texts, and texts that score nothing
    for rep in range(40):
        out.append((_rand_seq(rng, int(rng.integers(1, 200))), _rand_seq(rng, int(rng.integers(1, 260)))))
    for rep in range(8):
        out.append(("N" * int(rng.integers(1, 200)), _rand_seq(rng, int(rng.integers(1, 200)))))
        out.append((_rand_seq(rng, int(rng.integers(1, 200))), "N" * int(rng.integers(1, 200))))
    return out
