"""tests/polish_model.py against answers that follow from the constructions of tests/polish_cases.py alone (no GPU needed):
every record class and every column class occurs, the planned columns end as planned, planted errors under enough reads come
back as the truth, and -- the ground-truth claim -- a genome's contig with planted substitutions and N columns, under
error-free reads of both strands, is the genome again at every column the model does not report thin or uncovered, through
align_model, gap_model and polish_model in sequence."""
import numpy as np
import pytest

import align_model as A
import gap_model as G
import polish_cases as PC
import polish_model as M

NAMES = sorted(PC.BUILDERS)


def column_classes(c, want):
    """every column's class, recomputed from the counts the model returned"""
    out, counts, _, _, _ = want
    text = "".join(x + "_" for x in c.contigs)
    kw = dict(M.DEFAULTS, **c.kw)
    cls = {}
    for j, ch in enumerate(text):
        if ch != "_":
            cur = "ACGT".index(ch) if ch in "ACGT" else 4
            cls[j] = M.decide([int(x) for x in counts[j]], cur, kw["min_depth"], kw["min_permille"])[0]
    return cls


def test_every_record_class_and_every_column_class_occurs():
    seen = dict.fromkeys(M.RECORD_CLASSES + M.COLUMN_CLASSES + ("filled",), 0)
    for name in NAMES:
        st = PC.expected(name)[4]
        for k in seen:
            seen[k] += st[k]
    assert all(seen.values()), seen


@pytest.mark.parametrize("name", NAMES)
def test_outputs_agree_with_each_other(name):
    c = PC.case(name)
    out, counts, ctgs, fixes, st = PC.expected(name)
    text = "".join(x + "_" for x in c.contigs).encode()
    assert len(out) == len(text) and counts.shape == (len(text), 4) and len(ctgs) == len(c.contigs)
    diff = [j for j in range(len(text)) if out[j] != text[j]]
    assert diff == [int(p) for p in fixes["pos"]] and st["changed"] == len(diff)
    assert all(out[j] == ord("_") and not counts[j].any() for j, ch in enumerate(text) if ch == ord("_"))
    assert [bytes([int(f["old"])]) for f in fixes] == [text[int(f["pos"]):int(f["pos"]) + 1] for f in fixes]
    assert all(chr(int(f["new"])) in "ACGT" and f["new"] != f["old"] and f["pad"] == 0 for f in fixes)
    for k in ("votes", "placed", "changed", "filled", "disputed", "thin", "uncovered"):
        assert int(ctgs[k].sum()) == st[k], k
    cls = column_classes(c, (out, counts, ctgs, fixes, st))
    for k in M.COLUMN_CLASSES:
        assert sum(1 for v in cls.values() if v == k) == st[k], k
    assert st["sort_passes"] == (0 if not len(c.alns) else 3 if len(text) > 65535 else 2 if len(text) > 255 else 1)


def test_planned_columns():
    c = PC.case("columns")
    out, counts, ctgs, fixes, st = PC.expected("columns")
    cls = column_classes(c, (out, counts, ctgs, fixes, st))
    want = {"filled": "changed", "tie": "disputed", "at_depth": "changed", "below_depth": "thin", "at_permille": "changed",
            "short_of_permille": "disputed", "confirmed": "confirmed", "uncovered": "uncovered"}
    for name, (col, x) in c.plans.items():
        assert cls[col] == want[name], (name, counts[col])
        if want[name] == "changed":
            assert out[col] == ord(x)
        else:
            assert out[col] == ord(c.contigs[0][col])
    assert st["filled"] == 1 and sorted(int(counts[c.plans[n][0]].sum()) for n in ("at_depth", "below_depth")) == [3, 4]
    assert sorted(int(x) for x in counts[c.plans["at_permille"][0]]) == [0, 0, 2, 6]
    assert sorted(int(x) for x in counts[c.plans["short_of_permille"][0]]) == [0, 0, 3, 5]


def test_record_classes_by_construction():
    st = PC.expected("classes")[4]
    assert [st[k] for k in M.RECORD_CLASSES] == [1, 2, 2, 1, 1, 5]
    c = PC.case("classes")
    out, counts = PC.expected("classes")[:2]
    # edge_clip 5: the read at the contig's left end votes from column 0 on and stops 5 short of its inner end; the one at
    # the right end likewise; the inner read is clipped on both sides
    assert counts[0].sum() == 1 and counts[54].sum() == 1 and counts[55].sum() == 0
    assert counts[499].sum() == 1 and counts[445].sum() == 1 and counts[444].sum() == 0
    assert counts[224].sum() == 0 and counts[225].sum() == 1 and counts[274].sum() == 1 and counts[275].sum() == 0
    assert out[2] == ord(c.truth[0][2]) and out[497] == ord(c.truth[0][497])
    # without KC_POLISH_BEST_ONLY the two other records of the read at 280 are judged on their own
    free = M.polish(c.contigs, c.reads, c.alns, quals=c.quals, **dict(c.kw, best_only=False))[4]
    assert free["not_best"] == 0 and free["placed"] + free["divergent"] == st["placed"] + st["divergent"] + 2


def test_saturated_counts_keep_an_exact_decision():
    c = PC.case("deep")
    out, counts, ctgs, fixes, st = PC.expected("deep")
    assert st["placed"] == 66000 and int(counts.max()) == 65535 and st["votes"] == 66000 * 30
    assert [int(p) for p in fixes["pos"]] == [40, 41, 55] and all(int(f["top"]) == 65535 == int(f["tot"]) for f in fixes)
    assert out[35:65] == c.truth[0][35:65].encode() and st["filled"] == 1


@pytest.mark.parametrize("name", ("tiles", "strands", "long"))
def test_the_truth_comes_back_wherever_the_reads_are_deep_enough(name):
    c = PC.case(name)
    out, counts, _, _, st = PC.expected(name)
    truth = "".join(t + "_" for t in c.truth).encode()
    cls = column_classes(c, PC.expected(name))
    assert st["changed"] > 10
    for j, k in cls.items():
        if k in ("confirmed", "changed"):
            assert out[j] == truth[j], (j, counts[j])


def test_order_of_the_records_does_not_matter():
    c = PC.case("tiles")
    rows = list(c.rows)
    c.rng.__class__(7).shuffle(rows)
    got = M.polish(c.contigs, c.reads, np.array(rows, dtype=M.GAP_ALN_DTYPE), quals=c.quals, **c.kw)
    want = PC.expected("tiles")
    assert got[0] == want[0] and (got[1] == want[1]).all() and got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
    assert got[4] == want[4]


@pytest.mark.parametrize("seed", (41, 42, 43))
def test_ground_truth_through_align_gap_and_polish(seed):
    genome, ctg, reads, spots = PC.genome_case(seed)
    block, offs = A.join_block([ctg])
    alns = A.align_reads(A.Index(block, offs, 15), reads)[0]
    gapped = G.align_gapped([ctg], reads, alns)[0]
    out, counts, ctgs, fixes, st = M.polish([ctg], reads, gapped, min_depth=3, min_permille=700, max_mismatches=8)
    assert st["placed"] >= 0.9 * len(reads) and st["changed"] == len(spots) and st["filled"] == 2
    left_out = 0
    for j in range(len(genome)):
        if int(counts[j].sum()) >= 3:  # neither thin nor uncovered
            assert out[j] == ord(genome[j]), (j, counts[j])
        else:
            left_out += 1
    # every inner column is deep enough: a read starts every 5 bases on both strands, so only the first and the last 5
    # columns have fewer than three reads over them
    assert left_out <= 10 and [int(p) for p in fixes["pos"]] == spots
    assert out[5:-6].decode() == genome[5:-5]


def test_arguments_are_refused_as_the_library_refuses_them():
    c = PC.case("empty")
    for kw in (dict(edge_clip=1025), dict(min_depth=0), dict(min_permille=1001), dict(min_qual=256)):
        with pytest.raises(M.BadArg):
            M.polish(c.contigs, c.reads, c.alns, **kw)
    bad = PC.case("classes")
    rows = list(bad.rows)
    rows[3] = M.D.rec(len(bad.reads), 0, 0, 30)  # a read the call does not have
    with pytest.raises(M.BadRecord) as e:
        M.polish(bad.contigs, bad.reads, np.array(rows, dtype=M.GAP_ALN_DTYPE))
    assert e.value.index == 3
    with pytest.raises(M.TooManyFixes):
        M.polish(bad.contigs, bad.reads, bad.alns, quals=bad.quals, fix_capacity=PC.expected("classes")[4]["changed"] - 1, **bad.kw)
