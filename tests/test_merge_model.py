"""CPU checks of tests/merge_model.py, the restatement of the pair merge the GPU tests compare kc_merge_pairs with:
the hand-worked pairs of golden/merge_hand_cases.json, and the Q2Perror table the kernel holds."""
import json
import os
import re

import numpy as np
import pytest

import merge_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "merge_hand_cases.json")))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_case(case):
    b, q, o = M.interleave([case["pair"]])
    packed, offs, st = M.merge_pairs(b, q, o, case["qual_offset"], case["min_kmer_len"])
    for k, v in case["expect"].items():
        assert st[k] == v, (k, case["rule"])
    assert packed.tolist() == case["packed"]
    assert offs.tolist() == case["offsets"]
    assert {k: st[k] for k in case["stats"]} == case["stats"]
    assert st["out_reads"] == 2 - st["merged"] - 2 * st["dropped"]
    assert st["out_bases"] <= len(b)


def test_hand_cases_cover_the_rules():
    names = {c["name"] for c in CASES}
    for n in ("clean_overlap", "mate1_longer_start_i", "overlap_12", "overlap_11", "mismatches_6_of_20", "mismatches_7_of_20",
              "perror_at_limit", "perror_over_limit", "two_good_offsets", "good_after_found", "both_ns_twice", "ncount_over_3",
              "n_of_mate1_touched_unmerged", "n_in_mate2_tail", "lower_case_and_iupac", "both_short_dropped", "lengths_1_and_10",
              "quality_cap_and_floor"):
        assert n in names


def test_side_effect_and_quality_rules_by_hand():
    c = {x["name"]: x for x in CASES}
    # the N at the end of mate 1 was compared with a base by the overlap-11 trial: quality 0 in the unmerged output
    pk = c["n_of_mate1_touched_unmerged"]["packed"]
    assert pk[39] == 4 and all(b >> 3 == 31 for b in pk[:39])
    # mismatch of equal qualities: mate 1's base, quality floored at 2; a match of 30 + 15 capped at 41 (31 in the cache)
    pk = c["quality_cap_and_floor"]["packed"]
    assert pk[23] >> 3 == 2 and pk[27] >> 3 == 2 and pk[30] >> 3 == 31 and pk[0] >> 3 == 30 and pk[79] >> 3 == 15
    # the tail N of mate 2 keeps its quality (no trial compared it)
    pk = c["n_in_mate2_tail"]["packed"]
    assert pk[65] == 4 | (25 << 3)


def test_q2perror_table_is_the_kernels():
    src = open(os.path.join(HERE, "..", "mhm2_kmer_analysis_v2_amd", "csrc", "kc_merge.hpp")).read()
    body = re.search(r"kc_q2perror\[81\] = \{(.*?)\};", src, re.S).group(1)
    vals = [float(t) for t in body.replace("\n", " ").split(",") if t.strip()]
    assert vals == M.Q2PERROR and len(vals) == 81
    assert M.Q2PERROR[0] == 1.0 and M.Q2PERROR[20] == 0.01 and M.Q2PERROR[80] == 1e-08


def test_model_rejects_what_the_reference_dies_on():
    with pytest.raises(M.BadBase):
        M.merge_pairs(*M.interleave([("ACGTX" * 5, "I" * 25, "ACGT" * 6, "I" * 24)]))
    with pytest.raises(M.BadBase):
        M.merge_pairs(*M.interleave([("ACGT" * 6, "I" * 24, "ACGr" * 6, "I" * 24)]))
    with pytest.raises(M.BadArg):
        M.merge_pairs(*M.interleave([("ACGT" * 6, "I" * 23 + " ", "ACGT" * 6, "I" * 24)]))
    with pytest.raises(M.BadArg):
        M.merge_pairs(*M.interleave([("ACGT" * 6, "I" * 23 + chr(33 + 81), "ACGT" * 6, "I" * 24)]))


def test_random_pairs_stats_add_up():
    rng = np.random.default_rng(3)
    b, q, o = M.interleave(M.random_pairs(rng, 500))
    packed, offs, st = M.merge_pairs(b, q, o)
    assert st["out_reads"] == 2 * st["pairs"] - st["merged"] - 2 * st["dropped"]
    assert st["out_bases"] == len(packed) == int(offs[-1]) <= len(b)
    assert st["merged"] > 100 and st["ambiguous"] > 0 and st["dropped"] > 0
