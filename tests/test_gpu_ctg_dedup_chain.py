"""kc_ctg_dedup between kc_local_assm and the index: on the device's own blocks of tests/chain_cases.py's noisy construction
it equals tests/dedup_model.py, the seed index takes its output and loses no seed by it, kc_ctg_select and kc_fasta_text take
it, and a second pass removes nothing.  The unitigs of a counted read set go through unchanged: their k-mers occur once."""
import numpy as np
import pytest

import chain_cases as CC
import dedup_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from test_chain_model import SEEDS
from test_gpu_chain_noisy import Inputs, host, strings_of

pytestmark = pytest.mark.gpu

K = CC.K


def same_as_model(out, ctgs, depths=None, **kw):
    seqs, offsets, d, recs, st = out
    per = None
    if depths is not None:
        _, offs = M.block(ctgs)
        per = [depths[int(offs[u]):int(offs[u]) + len(c)] for u, c in enumerate(ctgs)]
    want = M.dedup(ctgs, K, depths=per, **kw)
    assert st == want["stats"], (st, want["stats"])
    assert host(seqs).tobytes() == want["seqs"].tobytes() and (host(offsets, np.uint64) == want["offsets"]).all()
    assert host(recs).tobytes() == want["records"].tobytes()
    if depths is not None:
        assert (host(d, np.uint16) == want["depths"]).all()
    return want


@pytest.fixture(scope="module")
def chain():
    """the counter with the case's contigs indexed, the reads on the device and local_assm's block"""
    case = CC.noisy_assembly(SEEDS[0])
    inp = Inputs(case)
    with pkg.KmerCounter(K) as kc:
        b, q, o, seqs, coffs = inp.on(True)
        kc.index_contigs(seqs, coffs)
        alns, _, _ = kc.align_reads(b, o)
        gapped, _ = kc.align_gapped(b, o, alns)
        _, pairs, _ = kc.pair_inserts(o, gapped, max_insert=CC.MAX_INSERT)
        _, ctgs, _ = kc.aln_depths(gapped)
        grown = kc.local_assm(b, q, o, gapped, pairs, ctg_depths=ctgs, max_insert=CC.MAX_INSERT)
        yield kc, case, inp, grown


def test_unitigs_go_through_unchanged():
    case = CC.noisy_assembly(SEEDS[0]).subset(150)
    inp = Inputs(case)
    b, q, o, _, _ = inp.on(True)
    with pkg.KmerCounter(K) as kc:
        kc.submit_reads(b, q, o)
        kc.flush()
        seqs, offsets, _, ust = kc.unitigs()
        _, depths = kc.unitig_block()
        assert ust["unitigs"] > 10
        out = kc.dedup_contigs(seqs, offsets, depths)
        st = out[4]
        assert st["candidates"] == 0 and st["kept"] == st["contigs"] == ust["unitigs"] and st["window_hits"] == st["anchored"] > 0
        assert host(out[0]).tobytes() == host(seqs).tobytes() and (host(out[1]) == host(offsets)).all() and (host(out[2]) == host(depths)).all()
        same_as_model(out, strings_of(host(seqs), host(offsets, np.uint64)), host(depths, np.uint16))


@pytest.mark.parametrize("kw", (dict(), dict(max_mismatches=2), dict(duplicates_only=True)), ids=("exact", "two mismatches", "duplicates only"))
def test_local_assm_block_against_the_model(chain, kw):
    kc, case, inp, grown = chain
    ctgs = strings_of(host(grown[0]), host(grown[1], np.uint64))
    same_as_model(kc.dedup_contigs(grown[0], grown[1], **kw), ctgs, **kw)
    # the same from host arrays
    same_as_model(kc.dedup_contigs(host(grown[0]), host(grown[1], np.uint64), **kw), ctgs, **kw)


def test_the_index_selection_and_text_take_the_result(chain):
    kc, case, inp, grown = chain
    # the case's own contigs overlap (draw_layout) but none lies in another; a planted copy and a planted slice do
    ctgs = strings_of(host(grown[0]), host(grown[1], np.uint64))
    assert len(ctgs[0]) > 200
    seqs, offsets = M.block(ctgs + [ctgs[0], M.rc(ctgs[1].encode())[10:150]])
    before = kc.index_contigs(seqs, offsets)
    out = kc.dedup_contigs(seqs, offsets)
    want = same_as_model(out, ctgs + [ctgs[0], M.rc(ctgs[1].encode())[10:150]])
    assert want["stats"]["duplicates"] >= 1 and want["stats"]["contained"] >= 1
    after = kc.index_contigs(out[0], out[1])
    assert after["contigs"] == out[4]["kept"] and after["repeated"] <= before["repeated"] and after["seeds"] >= before["seeds"]
    assert after["seeds"] > before["seeds"]  # the copies' k-mers are seeds again
    order, st = kc.select_contigs(out[0], out[1], by_length=True)
    assert st["contigs"] == st["selected"] == out[4]["kept"] and st["bases"] == out[4]["kept_bases"]
    text = kc.fasta_text(out[0], out[1], order)
    assert text.count(b">") == out[4]["kept"]
    # on its own output it removes nothing
    again = kc.dedup_contigs(out[0], out[1])
    assert again[4]["kept"] == again[4]["contigs"] == out[4]["kept"] and again[0].tobytes() == out[0].tobytes()
    kc.index_contigs(inp.seqs, inp.ctg_offsets)  # the fixture's index again


def test_device_tensors_through_the_index(chain):
    kc, case, inp, grown = chain
    out = kc.dedup_contigs(grown[0], grown[1])
    assert out[0].is_cuda and out[3].is_cuda
    before, after = kc.index_contigs(grown[0], grown[1]), kc.index_contigs(out[0], out[1])
    assert after["repeated"] <= before["repeated"] and after["seeds"] >= before["seeds"]
    again = kc.dedup_contigs(out[0], out[1])
    assert again[4]["kept"] == again[4]["contigs"] and host(again[0]).tobytes() == host(out[0]).tobytes()
    kc.index_contigs(*inp.on(True)[3:])
