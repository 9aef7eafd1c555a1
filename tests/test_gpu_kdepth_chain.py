"""The depth track in its place in the assembly chain: tests/chain_cases.py's noisy construction, the reads counted at k = 21,
the contigs extended by kc_local_assm and deduplicated by kc_ctg_dedup -- a block whose text matches no depth array any
more -- then contig_kmer_depths on that block from the table of the round, which is still resident.  The track equals the
model on the device's own block; after kc_reset to the next k the block and the track go into the contig pass, and what
kc_finalize gives equals the oracle fed the same reads and the same contigs with the model's mean as each one's depth."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import kdepth_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from oracle import cpu_oracle as O
from test_chain_model import SEEDS
from test_gpu_chain_noisy import Inputs, host, strings_of
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

K, NEXT_K = CC.K, 33


@pytest.mark.parametrize("device", (True, False), ids=("device", "host"))
def test_extended_deduplicated_contigs_get_their_depths_from_the_table(device):
    case = CC.noisy_assembly(SEEDS[0])
    inp = Inputs(case)
    b, q, o, seqs, coffs = inp.on(True)
    with pkg.KmerCounter(K) as kc:
        kc.submit_reads(b, q, o)
        keys, counts, _, _ = kc.sorted_results()
        kc.index_contigs(seqs, coffs)
        alns, _, _ = kc.align_reads(b, o)
        gapped, _ = kc.align_gapped(b, o, alns)
        _, pairs, _ = kc.pair_inserts(o, gapped, max_insert=CC.MAX_INSERT)
        _, ctgs, _ = kc.aln_depths(gapped)
        l_seqs, l_offsets, ends, lst = kc.local_assm(b, q, o, gapped, pairs, ctg_depths=ctgs, max_insert=CC.MAX_INSERT)
        assert lst["ext_bases"] > 0 and int(l_seqs.numel()) > int(seqs.numel())
        d_seqs, d_offsets, _, _, dst = kc.dedup_contigs(l_seqs, l_offsets)
        h_seqs, h_offsets = host(d_seqs), host(d_offsets, np.uint64)
        args = (d_seqs, d_offsets) if device else (h_seqs, h_offsets)
        depths = kc.contig_kmer_depths(*args)
        # ---- the model on the device's own block, from the results of the round
        want_track, want_recs, _ = M.kmer_depths(M.table(keys, counts, K), K, h_seqs, h_offsets, fill_mean=True)
        assert (host(depths, np.uint16) == want_track).all() and want_recs["mean"].max() >= 2 and len(want_recs) == dst["kept"] > 3
        assert (want_track[h_offsets[1:].astype(np.int64) - 1] == 0).all()  # the separators
        # ---- the next round takes the block and the track as they are
        kc.reset(NEXT_K)
        kc.submit_reads(b, q, o)
        kc.begin_ctg_kmers(int(d_seqs.numel()))
        kc.submit_ctg_block(d_seqs, depths if device else torch.from_numpy(depths.view(np.int16)).cuda())
        got = kc.sorted_results()
    orc = O.Oracle(NEXT_K)
    orc.add_reads(inp.bases, inp.quals, inp.offsets)
    for text, rec in zip(strings_of(h_seqs, h_offsets), want_recs):
        orc.add_ctg(text, int(rec["mean"]))
    want = orc.finalize()
    orc.close()
    assert_same(got, want)
