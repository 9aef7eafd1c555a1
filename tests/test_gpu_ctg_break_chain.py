"""Index, align, align gapped, classify the pairs, break, index the pieces, align again: the chimeric contig of
tests/break_cases.py's chain case through kc_ctg_break on the device.  Two random genomes of 5000 bases;
contig 0 is the left half of the first joined to the right half of the second, contigs 1 and 2 the halves left over; 2000
noisy pairs.  The break equals tests/break_model.py on the device's own gapped records and pair records, device tensors and host
arrays.  The ground truth is the one tests/test_break_model.py establishes through the host models for the same seed: exactly
one break, in the chimeric contig, at most one read length from the junction, the true contigs unbroken.  Then the new block
is indexed and the reads aligned again: every pair with a mate on a piece of the chimeric contig is now proper or has its mates
on two contigs."""
import numpy as np
import pytest

import break_cases as BC
import break_model as M
import depth_model as DM
import gap_model as GM
import mhm2_kmer_analysis_v2_amd as pkg
from links_cases import K, READ_LEN
from test_gpu_chain_noisy import Inputs, host
from test_gpu_ctg_break import same

pytestmark = pytest.mark.gpu


def test_align_break_index_again_and_align():
    case = BC.chain_case()
    inp = Inputs(case)
    b, q, o, seqs, coffs = inp.on(True)
    with pkg.KmerCounter(K) as kc:
        kc.index_contigs(seqs, coffs)
        alns, _, _ = kc.align_reads(b, o)
        gapped, _ = kc.align_gapped(b, o, alns)
        _, pairs, ist = kc.pair_inserts(o, gapped, max_insert=BC.CHAIN_INSERT)
        depths, _, _ = kc.aln_depths(gapped)
        h_gapped, h_pairs, h_depths = host(gapped, GM.GAP_ALN_DTYPE), host(pairs, DM.PAIR_DTYPE), host(depths, np.uint16)
        # ---- the break, on the device's records: device tensors and host arrays against the model
        want = M.break_contigs(case.contigs, case.read_lens, h_gapped, h_pairs, depths=h_depths, **BC.CHAIN_KW)
        got = kc.break_contigs(o, gapped, pairs, depths=depths, tracks=True, **BC.CHAIN_KW)
        same(got, want)
        same(kc.break_contigs(inp.offsets, h_gapped, h_pairs, depths=h_depths, tracks=True, **BC.CHAIN_KW), want)
        # ---- the ground truth
        st, brk = want[5], want[4]
        assert st["breaks"] == 1 and st["broken_contigs"] == 1 and int(brk[0]["ctg"]) == 0 and st["pieces"] == 4
        pos = int(brk[0]["pos"])
        print("the break at %d, the junction at %d: %d apart; %s" % (pos, case.junction, abs(pos - case.junction), st))
        assert abs(pos - case.junction) <= READ_LEN
        assert [tuple(int(x) for x in p) for p in want[3]] == [(0, 0, pos, 2), (0, pos, 5000 - pos, 1), (1, 0, 2500, 0), (2, 0, 2500, 0)]
        pieces = want[0].decode().split("_")[:-1]
        assert pieces == [case.contigs[0][:pos], case.contigs[0][pos:], case.contigs[1], case.contigs[2]]
        # ---- the new block is a contig block: index it on the device and align again
        info = kc.index_contigs(got[0], got[1])
        assert kc.contig_index_info() == (len(want[0]), 4) and info["contigs"] == 4
        alns2, _, _ = kc.align_reads(b, o)
        gapped2, _ = kc.align_gapped(b, o, alns2)
        _, pairs2, ist2 = kc.pair_inserts(o, gapped2, max_insert=BC.CHAIN_INSERT)
        g2, p2 = host(gapped2, GM.GAP_ALN_DTYPE), host(pairs2, DM.PAIR_DTYPE)
        on_chimera = lambda i: i != M.NO_ALN and int(g2[i]["ctg"]) in (0, 1)  # noqa: E731
        touched = [p for p in p2 if on_chimera(int(p["aln0"])) or on_chimera(int(p["aln1"]))]
        assert len(touched) > 500 and all(int(p["cls"]) in (DM.PAIR_DIFF_CTG, DM.PAIR_PROPER) for p in touched)
