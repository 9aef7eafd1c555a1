"""tests/trim_model.py's aligner against the reference's own: every case of tests/golden/ssw_ref_alignments.json (made by
tests/golden/make_ssw_golden.py from the reference's src/ssw, compiled unmodified) in all five recorded fields, for both
score sets.  No case is left out."""
import json
import os

import pytest

import trim_model as M
from golden.make_ssw_golden import FIELDS, SETS, inputs_sha256

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLD, "ssw_ref_alignments.json")))


@pytest.fixture(scope="module")
def adapters():
    return M.read_fasta_seqs(os.path.join(GOLD, "adapters_no_transposase.fa"))


@pytest.mark.parametrize("name,blastn", SETS)
def test_aligner_equals_reference(golden, adapters, name, blastn):
    g = golden["sets"][name]
    cases = M.ssw_cases(adapters, blastn)
    assert len(cases) == g["n"] and len(cases) >= 4000
    assert inputs_sha256(cases) == g["inputs_sha256"], "the seeded inputs are not those the reference answered"
    rows = [[int(v) for v in r.split(",")] for r in g["results"].split(" ")]
    assert len(rows) == len(cases)
    scores = M.SCORES_BLASTN if blastn else M.SCORES_ALTERNATE
    bad = []
    for (q, r), row in zip(cases, rows):
        got = M.ssw_align(q.encode(), r.encode(), scores)
        if [got[f] for f in FIELDS] != row:
            bad.append((q, r, row, got))
    assert not bad, "%d of %d cases differ, first: %r" % (len(bad), len(cases), bad[0])
    if blastn:  # the recorded cases cross the byte lanes' limit (max + bias >= 255, bias 3) both ways
        assert sum(1 for row in rows if row[0] + 3 >= 255) > 50 and sum(1 for row in rows if 200 <= row[0] + 3 < 255) > 50


def test_loader_corners():
    a = M.AdapterSet(b">x\nACGTACGTACGTACGTACGTAC\n\nACGT\n>y\nTTTTTTTTTTTTTTTTTTTTTTTTT", 21)
    assert a.n_adapters == 2 and a.n_short == 2 and len(a.entries) == 4
    assert a.entries[1] == b"GTACGTACGTACGTACGTACGT" and a.entries[3] == b"A" * 25
    assert a.index[bytes([3] * 21)] == [(2, j) for j in range(5)]
    with pytest.raises(M.BadBase):
        M.AdapterSet(b">x\nACGTACGTACGTACGTACGTAC\r\n", 21)
    with pytest.raises(M.UnsupportedK):
        M.AdapterSet(b"", 33)


def test_trim_rules_by_hand():
    ad = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"
    a = M.AdapterSet((">a\n%s\n" % ad).encode(), 21)
    ins = "TTGACCATGCATTGCAAGGCTTACGGATCCATGCAAGTTCAGG"
    assert M.trim(a, (ins + ad).encode()) == (len(ins), True, 1)
    assert M.trim(a, (ins[:11] + ad).encode()) == (0, True, 1)       # a cut below 12 removes the read
    assert M.trim(a, (ins[:12] + ad).encode()) == (12, True, 1)
    assert M.trim(a, ins.encode()) == (len(ins), False, 0)
    assert M.trim(a, ad[:20].encode()) == (20, False, 0)             # shorter than k: left alone
    b, q, o, st = M.trim_reads(a, list((ins + ad + ins).encode()), [40] * (2 * len(ins) + len(ad)), [0, len(ins) + len(ad), 2 * len(ins) + len(ad)], True)
    assert list(o) == [0, len(ins), 2 * len(ins)] and st["trimmed"] == 1 and st["bases_trimmed"] == len(ad)
