"""Index, align, align gapped, polish, index the polished block, align again: tests/chain_cases.py's noisy read pairs through
kc_ctg_polish on the device.  The case's contigs are pieces of its genome; a substitution is planted in
them every 97 bases before they are indexed.  Every step equals its model on the device's own previous output: align_model
on the planted contigs, gap_model on the device's records, polish_model on the device's gapped records, align_model again on
the device's polished block.  The first SUBSET pairs only: gap_model's dynamic programme in Python is what the test costs.
The planted errors restored and the bytes changed wrongly are printed, and follow from the model alone; no figure is fixed
here beyond the device being the model."""
import numpy as np
import pytest

import align_model as A
import chain_cases as NC
import gap_model as GM
import polish_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from test_chain_model import SEEDS
from test_gpu_chain_noisy import Inputs, dev, host, same_records
from test_gpu_polish import same

pytestmark = pytest.mark.gpu

SUBSET = 150
KW = dict(min_depth=3, min_permille=700, max_mismatches=8, min_qual=10, edge_clip=2)


def plant(contigs, every=97):
    out, spots = [], []
    for u, c in enumerate(contigs):
        t = list(c)
        for p in range(every // 2, len(t), every):
            if t[p] in "ACGT":
                t[p] = "ACGT"[("ACGT".index(t[p]) + 1 + (p + u) % 3) % 4]
                spots.append((u, p))
        out.append("".join(t))
    return out, spots


@pytest.mark.parametrize("seed", SEEDS[:1])
def test_align_polish_index_again_and_align(seed):
    full = NC.noisy_assembly(seed)
    case = full.subset(SUBSET)
    contigs, spots = plant(case.contigs)
    planted = NC.Case(**dict(case.__dict__, contigs=contigs))
    inp = Inputs(planted)
    b, q, o, seqs, coffs = inp.on(True)
    quals = [x.encode() for x in case.quals]
    with pkg.KmerCounter(NC.K) as kc:
        kc.index_contigs(seqs, coffs)
        alns, first, ast = kc.align_reads(b, o)
        index = A.Index(*A.join_block(contigs), NC.K)
        want_alns = A.align_reads(index, case.reads)
        same_records(host(alns, A.ALN_DTYPE), want_alns[0], "align_reads")
        gapped, gst = kc.align_gapped(b, o, alns)
        h_gapped = host(gapped, GM.GAP_ALN_DTYPE)
        want_gapped, want_gst = GM.align_gapped(contigs, case.reads, host(alns, A.ALN_DTYPE))
        same_records(h_gapped, want_gapped, "align_gapped")
        assert gst == want_gst
        # ---- the polish, on the device's records, device tensors and host arrays
        want = M.polish(contigs, case.reads, h_gapped, quals=quals, **KW)
        got = kc.polish_contigs(b, o, gapped, quals=q, with_counts=True, **KW)
        same(got, want)
        same(kc.polish_contigs(inp.bases, inp.offsets, h_gapped, quals=inp.quals, with_counts=True, **KW), want)
        polished = want[0].decode().split("_")[:-1]
        assert [len(x) for x in polished] == [len(x) for x in contigs] and want[4]["changed"] > 0
        restored = sum(1 for u, p in spots if polished[u][p] == case.contigs[u][p])
        wrong = sum(1 for u, c in enumerate(polished) for p in range(len(c)) if c[p] != contigs[u][p] and c[p] != case.contigs[u][p])
        print("planted %d, restored %d, changed %d, changed wrongly %d; %s" % (len(spots), restored, want[4]["changed"], wrong, want[4]))
        # ---- the polished block is a contig block: index it, on the device, and align again
        info = kc.index_contigs(got[0], coffs)
        again = A.Index(*A.join_block(polished), NC.K)
        assert info == again.stats
        alns2, first2, ast2 = kc.align_reads(b, o)
        want2 = A.align_reads(again, case.reads)
        same_records(host(alns2, A.ALN_DTYPE), want2[0], "align_reads on the polished block")
        assert ast2 == want2[2] and (host(first2, np.uint64) == want2[1]).all()
        # lengths and offsets are the first block's: the first round's records still index the polished block
        st = kc.aln_depths(gapped)[2]
        assert st["records"] == len(h_gapped)
