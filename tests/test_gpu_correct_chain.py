"""Count, correct, count again, align: tests/chain_cases.py's noisy read pairs through kc_correct_reads on the device (DESIGN.md
section 32).  The corrected reads are the model's byte for byte; counted again after kc_reset they fill the table with no more
k-mers than before (kc_stats.num_unique, the table's entries before the purge: 32 464 -> 15 081 at seed 32; the results grow
by the few true k-mers that are seen twice only once the reads are corrected, 11 590 -> 11 609, which the test does not
bound from above by the first count); aligned to the case's contigs they leave a share of kc_align_gapped records to the
dynamic programme that is no greater than before (0.73 -> 0.19).  Both inequalities hold in the model chain
(tests/test_correct_model.py); no figure is fixed here."""
import numpy as np
import pytest

import chain_cases as NC
import correct_model as M
import kdepth_model as K
import mhm2_kmer_analysis_v2_amd as pkg
from test_chain_model import SEEDS
from test_gpu_chain_noisy import Inputs
from test_gpu_correct_reads import same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", SEEDS)
def test_count_correct_count_again_and_align(seed):
    case = NC.noisy_assembly(seed)
    inp = Inputs(case)
    b, q, o, seqs, coffs = inp.on(True)
    with pkg.KmerCounter(NC.K) as kc:
        kc.submit_reads(inp.bases, inp.quals, inp.offsets)
        keys, counts = kc.sorted_results()[:2]
        before = kc.stats()
        want = M.correct_reads(K.table(keys, counts, NC.K), NC.K, inp.bases, inp.offsets)
        got = kc.correct_reads(b, o, with_fixes=True)
        same(got, want)
        same(kc.correct_reads(inp.bases, inp.offsets, quals=inp.quals, with_fixes=True), want)  # max_qual 0: the qualities are not looked at
        assert want[3]["accepted"] > 500
        fixed = got[0]
        # ---- the share of the dynamic programme, on the case's contigs
        kc.index_contigs(seqs, coffs)
        share = []
        for bases in (b, fixed):
            alns = kc.align_reads(bases, o)[0]
            st = kc.align_gapped(bases, o, alns)[1]
            print("align_gapped", st)
            share.append(st["dp"] / st["records"])
        assert share[1] <= share[0]
        # ---- the second count
        kc.reset()
        kc.submit_reads(fixed, q, o)
        kc.finalize()
        after = kc.stats()
        print("num_unique", before["num_unique"], after["num_unique"], "total_kmers", before["total_kmers"], after["total_kmers"])
        assert after["num_unique"] <= before["num_unique"] and after["num_reads"] == before["num_reads"]
        # and the corrected reads hold no more weak windows in their own table than the noisy ones did in theirs
        again = kc.kmer_depths(fixed, o, min_count=2)[2]
        assert again["windows"] - again["solid"] <= want[3]["weak_before"]
