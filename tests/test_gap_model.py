"""tests/gap_model.py, the host model of kc_align_gapped (no GPU needed): its dynamic programme against what the
reference's own aligner answered for read-sized inputs (tests/golden/gap_ref_alignments.json, written by
tests/golden/make_gap_golden.py), the step around it on hand cases with the answers written out
(tests/golden/gap_hand_cases.json), and the model behind tests/align_model.py's align_reads."""
import hashlib
import json
import os

import numpy as np
import pytest

import align_model as A
import gap_model as G
import trim_model as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("sw_score", "ref_begin", "ref_end", "query_begin", "query_end")


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


@pytest.mark.parametrize("name", ["11111", "23521", "13521"])
def test_dynamic_programme_against_the_reference_aligner(name):
    gold = json.load(open(os.path.join(GOLDEN, "gap_ref_alignments.json")))
    assert gold["fields"] == list(FIELDS) and sorted(gold["sets"]) == sorted(G.SCORE_SETS)
    g = gold["sets"][name]
    cases = G.gap_ssw_cases(name)
    h = hashlib.sha256()
    for q, r in cases:
        h.update(q.encode() + b" " + r.encode() + b"\n")
    assert len(cases) == g["n"] and h.hexdigest() == g["inputs_sha256"], "the seeded inputs are not the recorded ones"
    rows = [[int(v) for v in row.split(",")] for row in g["results"].split(" ")]
    assert len(rows) == len(cases)
    lengths = {len(q) for q, _ in cases}
    cap = G.CAP_11111 if name == "11111" else A.MAX_READ_LEN
    assert {min(L, cap) for L in G.NAMED_LENGTHS} <= lengths and max(lengths) == cap
    bad = []
    for i, ((q, r), row) in enumerate(zip(cases, rows)):
        got = T.ssw_align(q.encode(), r.encode(), G.SCORE_SETS[name])
        if [got[f] for f in FIELDS] != row:
            bad.append((i, row, got))
    assert not bad, bad[:5]


def test_hand_cases():
    hand = json.load(open(os.path.join(GOLDEN, "gap_hand_cases.json")))
    assert tuple(hand["scores"]) == G.SCORES_BLASTN
    assert len(hand["cases"]) >= 5
    for case in hand["cases"]:
        alns = np.zeros(1, dtype=A.ALN_DTYPE)
        for k, v in case["record"].items():
            alns[0][k] = v
        out, st = G.align_gapped([hand["contig"]], [case["read"]], alns, hand["pad"], tuple(hand["scores"]))
        got = {k: int(out[0][k]) for k in case["want"]}
        assert got == case["want"], case["name"]
        assert (int(out[0]["read"]), int(out[0]["ctg"]), int(out[0]["orient"]), int(out[0]["seeds"])) == \
            (0, 0, case["record"]["orient"], case["record"]["seeds"])
        assert st["records"] == 1 and st["score_sum"] == case["want"]["score"]
        if "in the middle" in case["name"]:  # 150 rows, and the diagonal's 150 columns with 16 on either side
            assert st["cells"] == 150 * 182 and st["dp"] == 1
    # the two indel cases as the issue states them: the whole read, 2 * matched bases less the gap
    dele, ins = hand["cases"][0]["want"], hand["cases"][1]["want"]
    assert (dele["rstart"], dele["rstop"], dele["score"]) == (0, 150, 2 * 150 - 7)
    assert (ins["rstart"], ins["rstop"], ins["score"]) == (0, 150, 2 * 149 - 5)


def test_rules_around_the_dynamic_programme():
    rng = np.random.default_rng(3)
    ctg = rand_seq(rng, 200)
    read = ctg[20:120]

    def rec(**kw):
        a = np.zeros(1, dtype=A.ALN_DTYPE)
        base = dict(read=0, ctg=0, orient=0, cstart=20, cstop=120, rstart=0, rstop=100, seeds=3, mismatches=77)
        base.update(kw)
        for k, v in base.items():
            a[0][k] = v
        return a

    out, st = G.align_gapped([ctg], [read], rec(), 16, G.SCORES_ALTERNATE)
    assert (int(out[0]["kind"]), int(out[0]["score"]), int(out[0]["mismatches"])) == (G.KIND_EXACT, 100, 0)  # the input's 77 is not read
    assert st == dict(records=1, exact=1, dp=0, none=0, cells=0, score_sum=100)
    out, st = G.align_gapped([ctg], [read], rec(), 16, G.SCORES_BLASTN, always_dp=True)
    assert (int(out[0]["kind"]), int(out[0]["score"]), int(out[0]["cstart"]), int(out[0]["cstop"])) == (G.KIND_DP, 200, 20, 120)
    assert st == dict(records=1, exact=0, dp=1, none=0, cells=100 * 132, score_sum=200)
    # U is no base here (kBaseTranslation would make it an A); lower case is a base
    u = read[:50].lower() + "U" + read[51:]
    out, _ = G.align_gapped([ctg], [u], rec(), 16, G.SCORES_BLASTN)
    assert int(out[0]["mismatches"]) == 1 and int(out[0]["score"]) == 2 * 99 - 1
    # a forged diagonal that passes the checks and scores nothing; an all-N read
    forged = rec(cstart=0, cstop=1, rstart=99, rstop=100)
    poly = "A" * 100
    out, st = G.align_gapped(["C" * 30], [poly], forged, 0, G.SCORES_BLASTN)
    assert out[0].tobytes()[8:24] == bytes(16) and int(out[0]["kind"]) == G.KIND_NONE and int(out[0]["mismatches"]) == 1
    assert st == dict(records=1, exact=0, dp=0, none=1, cells=100 * 1, score_sum=0)
    out, _ = G.align_gapped([ctg], ["N" * 100], rec(), 16, G.SCORES_BLASTN)
    assert int(out[0]["kind"]) == G.KIND_NONE and int(out[0]["mismatches"]) == 100
    # invalid records: the lowest index is named
    for bad in (rec(read=1), rec(ctg=1), rec(orient=2), rec(cstop=121), rec(rstop=101), rec(cstart=21, rstart=1), rec(cstop=119, rstop=99),
                rec(cstart=120, cstop=120, rstart=100, rstop=100), rec(cstart=20, cstop=119, rstart=1, rstop=100)):
        both = np.concatenate([rec(), bad, bad])
        with pytest.raises(G.BadRecord) as e:
            G.align_gapped([ctg], [read], both, 16, G.SCORES_BLASTN)
        assert e.value.index == 1
    for scores in ((0, 1, 1, 1, 1), (10, 1, 1, 1, 1), (1, 10, 1, 1, 1), (1, 1, 1, 2, 1), (1, 1, 1, 0, 1), (1, 1, 10, 1, 1), (1, 1, 1, 1, 10)):
        with pytest.raises(G.BadArg):
            G.align_gapped([ctg], [read], rec(), 16, scores)
    with pytest.raises(G.BadArg):
        G.align_gapped([ctg], [read], rec(), 1025, G.SCORES_BLASTN)
    with pytest.raises(G.BadArg):
        G.align_gapped([ctg], [read, "A" * 1025], rec(), 16, G.SCORES_BLASTN)


def test_behind_align_reads():
    """Reads with planted indels through align_model.align_reads, then through the model: the two diagonals of a read
    with one indel both refine to the one alignment of the whole read."""
    k = 21
    rng = np.random.default_rng(4)
    contigs = [rand_seq(rng, 500), rand_seq(rng, 400)]
    ix = A.Index(*A.join_block(contigs), k)
    c0, c1 = contigs
    reads = [c0[100:250],                                   # exact
             c0[100:175] + c0[177:252],                     # a 2-base deletion
             A.revcomp(c1[50:125] + "A" + c1[125:199]),     # a 1-base insertion, other strand
             c1[300:] + rand_seq(rng, 50)]                  # over the end: exact over its overlap
    alns, first, _ = A.align_reads(ix, reads)
    assert list(np.diff(first.astype(np.int64))) == [1, 2, 2, 1]
    out, st = G.align_gapped(contigs, reads, alns, 16, G.SCORES_BLASTN)
    assert [int(x) for x in out["kind"]] == [0, 1, 1, 1, 1, 0]
    for i in (1, 2):
        assert (int(out[i]["cstart"]), int(out[i]["cstop"]), int(out[i]["rstart"]), int(out[i]["rstop"]), int(out[i]["score"])) == \
            (100, 252, 0, 150, 293)
    for i in (3, 4):
        assert (int(out[i]["cstart"]), int(out[i]["cstop"]), int(out[i]["rstart"]), int(out[i]["rstop"]), int(out[i]["orient"])) == \
            (50, 199, 0, 150, 1)
        assert int(out[i]["score"]) in (2 * 149 - 5, 2 * 148 - 5 + 2)  # the inserted A may match a neighbour: still one gap
    assert (out["read"] == alns["read"]).all() and (out["seeds"] == alns["seeds"]).all() and not out["pad"].any()
    assert st["records"] == 6 and st["exact"] == 2 and st["dp"] == 4 and st["cells"] == 4 * 150 * 182
    # the records in another order: the same records in that order, the same statistics
    perm = np.array([4, 0, 5, 2, 1, 3])
    out2, st2 = G.align_gapped(contigs, reads, alns[perm], 16, G.SCORES_BLASTN)
    assert out2.tobytes() == out[perm].tobytes() and st2 == st
