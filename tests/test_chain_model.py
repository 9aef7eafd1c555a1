"""The host models as one chain over tests/chain_cases.py's noisy construction: align_model -> gap_model ->
depth_model.pair_inserts / aln_depths -> lassm_model -> links_model -> scaffold_model -> close_model -> shuffle_model ->
asm_model.select / fasta -> fasta_in_model.parse, every model on the output of the one before it.  No device.

Two kinds of claims.  The ground truth: what the chain ends in is the genome the case was cut from (chain_cases.check_*).
The path coverage: the case is not easy -- every figure of coverage() is non-zero, so the records of kind DP, the
repeated seeds, the pair classes, the far spans, the checked and the rejected overlaps, the off-join candidates and the
disputed columns are all there for tests/test_gpu_chain_noisy.py to compare the device on.

SEEDS: each of the two carries every figure of coverage() and every ground-truth claim on its own (of seeds 1 .. 89 eight carry
the figures and seven of those the claims; a closed scaffold misses the genome where two of four splint reads share a
substitution).  32 has 16 contigs in 2 scaffolds; 82 has 11, and a consensus column on which the votes tie."""
import time

import numpy as np
import pytest

import align_model as A
import asm_model as AM
import chain_cases as CC
import close_model as CM
import depth_model as D
import fasta_in_model as FM
import gap_model as GM
import lassm_model as LM
import links_model as KM
import scaffold_model as SM
import shuffle_model as SH
from test_gpu_gap_align import read_arrays

SEEDS = (32, 82)


def model_chain(case):
    """every model's result under its step's name, and the wall time of each step"""
    c, out, times = case, {}, {}

    def step(name, fn):
        t = time.perf_counter()
        out[name] = fn()
        times[name] = time.perf_counter() - t

    lens, rlens = c.ctg_lens, c.read_lens
    bases, offsets = read_arrays(c.reads)
    step("index", lambda: A.Index(*A.join_block(c.contigs), CC.K))
    step("align", lambda: A.align_reads(out["index"], c.reads))
    step("gapped", lambda: GM.align_gapped(c.contigs, c.reads, out["align"][0]))
    g = out["gapped"][0]
    step("pairs", lambda: D.pair_inserts(lens, rlens, g, max_insert=CC.MAX_INSERT))
    p = out["pairs"][1]
    step("depths", lambda: D.aln_depths(lens, g))
    step("lassm", lambda: LM.local_assm(c.contigs, c.reads, c.quals, g, p, out["depths"][1]["mean"], k=CC.K))
    step("links", lambda: KM.ctg_links(lens, rlens, g, p, **CC.LINK_KW))
    step("scaffolds", lambda: SM.scaffold(c.contigs, out["links"][0]))
    s = out["scaffolds"]
    step("closed", lambda: CM.close_gaps(c.contigs, c.reads, g, s[2], s[3], **CC.CLOSE_KW))
    step("shuffled", lambda: SH.shuffle_reads(lens, bases.tobytes(), "".join(c.quals).encode(), offsets, g, p, 3))
    seqs, offs = np.frombuffer(out["closed"][0], dtype=np.uint8), out["closed"][1]
    step("select", lambda: AM.select(seqs, offs, 500, True))
    step("fasta", lambda: AM.fasta(seqs, offs, None, "scaffold_", 60))
    step("parsed", lambda: FM.parse(out["fasta"]))
    return out, times


def coverage(out):
    """the figures that must not be zero, by name"""
    gst, ast, ist, lst, sst, cst = out["gapped"][1], out["align"][2], out["pairs"][2], out["links"][2], out["scaffolds"][5], out["closed"][5]
    members, scafs = out["scaffolds"][3], out["scaffolds"][2]
    return {"dp": gst["dp"], "exact": gst["exact"], "repeated_hits": ast["repeated_hits"],
            "insert classes beyond two": max(0, sum(1 for x in ist["cls"] if x) - 2), "spans_too_far": lst["spans_too_far"],
            "overlaps_checked": sst["overlaps_checked"], "overlaps_rejected": sst["overlaps_rejected"], "cands_off_join": cst["cands_off_join"],
            "disputed_cols": cst["disputed_cols"], "lassm statuses beyond one": sum(1 for x in out["lassm"][3]["status"] if x) - 1,
            "scaffolds beyond one": sst["scaffolds"] - 1,
            "scaffolds with a reversed member": sum(1 for x in scafs if int(x["n_members"]) > 1 and any(
                int(m["orient"]) for m in members[int(x["first_member"]):int(x["first_member"]) + int(x["n_members"])])),
            "reads with two records or more": int((np.diff(out["align"][1].astype(np.int64)) > 1).sum()),
            "clipped dp records": int(((out["gapped"][0]["kind"] == GM.KIND_DP) & (out["gapped"][0]["rstop"] - out["gapped"][0]["rstart"] < CC.READ_LEN)).sum())}


@pytest.fixture(scope="module", params=SEEDS)
def chain(request):
    case = CC.noisy_assembly(request.param)
    out, times = model_chain(case)
    print("seed %d: model chain %.1f s, of which align_gapped %.1f s on %d records" % (request.param, sum(times.values()), times["gapped"],
                                                                                      len(out["gapped"][0])))
    return case, out


def test_the_construction_is_what_it_says(chain):
    case, _ = chain
    (a0, a1), (b0, b1) = case.repeat
    assert case.G[a0:a1] == case.G[b0:b1] and abs(a0 - b0) >= 3000 and a1 - a0 == 300
    assert all(300 <= e - s <= 1500 for s, e, _ in case.layout) and all(-30 <= g <= 40 for g in case.gaps)
    assert 0 in case.gaps and min(case.gaps) < -CC.K and len({r for _, _, r in case.layout}) == 2
    assert [case.layout[i + 1][0] - case.layout[i][1] for i in range(len(case.gaps))] == case.gaps
    assert case.layout[0][0] == 0 and case.layout[-1][1] == len(case.G) == 12000
    assert all(len(r) == len(q) == CC.READ_LEN for r, q in zip(case.reads, case.quals)) and len(case.reads) == 2 * 410
    placed = [w for w in case.truth if w is not None]
    assert sum(1 for w in placed if w[3][1]) >= 10 and sum(w[3][0] for w in placed) >= 600
    assert sum("N" in r.upper() for r in case.reads) >= 5 and sum(r.islower() for r in case.reads) >= 5
    assert len({q for qs in case.quals for q in qs}) >= 10
    # a placed read without noise is the genome's text
    for r, w in zip(case.reads, case.truth):
        if w is not None and w[3] == (0, 0) and "N" not in r.upper():
            piece = case.G[w[0]:w[1]]
            assert r.upper() == (CC.revc(piece) if w[2] else piece)
    # the chimeric pairs and the pairs with a mate from nowhere
    far = sum(1 for p in range(len(case.reads) // 2) if None not in case.truth[2 * p:2 * p + 2]
              and abs(case.truth[2 * p][0] - case.truth[2 * p + 1][0]) > CC.MAX_INSERT)
    assert far == 6 and sum(w is None for w in case.truth) == 4


def test_path_coverage(chain):
    """every figure of coverage() is non-zero: the case holds what the chain's stages meet on real data"""
    _, out = chain
    cov = coverage(out)
    print(cov)
    print("gapped", out["gapped"][1], "\nalign", out["align"][2], "\ninserts", out["pairs"][2]["cls"], "\nlinks", out["links"][2],
          "\nscaffolds", out["scaffolds"][5], "\nclosed", out["closed"][5], "\nlassm", out["lassm"][3])
    assert all(v > 0 for v in cov.values()), {k: v for k, v in cov.items() if v <= 0}


def test_gapped_records_lie_on_the_true_diagonals(chain):
    case, out = chain
    checked, skipped = CC.check_gapped(case, out["gapped"][0])
    assert checked > 600 and skipped > 0


def test_links_join_the_layouts_neighbours(chain):
    case, out = chain
    checked, _ = CC.check_links(case, out["links"][0])
    assert checked >= len(case.gaps) // 2


def test_local_assembly_extends_into_the_genome(chain):
    case, out = chain
    block, offsets, ends, st = out["lassm"]
    assert CC.check_local_assm(case, block, offsets, ends) >= len(case.contigs) and st["ctgs_extended"] > 0


def test_closed_scaffolds_are_pieces_of_the_genome(chain):
    case, out = chain
    closed = out["closed"]
    CC.check_closed(case, CM.strings(closed), closed[5])
    assert closed[5]["filled"] > 0 and sum(len(s) for s in CM.strings(closed)) > 0.9 * len(case.G)


def test_fasta_round_trip_and_selection(chain):
    _, out = chain
    closed, parsed = out["closed"], out["parsed"]
    assert parsed["status"] == FM.OK and parsed["seqs"].tobytes() == closed[0] and (parsed["offsets"] == closed[1]).all()
    order, st = out["select"]
    lens = [len(s) for s in CM.strings(closed)]
    assert [lens[u] for u in order] == sorted((n for n in lens if n >= 500), reverse=True) and st["n"] == 0


def test_the_shuffle_keeps_every_pair(chain):
    case, out = chain
    s = out["shuffled"]
    order = np.frombuffer(s["order"], dtype=np.uint32)
    assert sorted(order.tolist()) == list(range(len(case.reads) // 2)) and s["stats"]["one_mate"] > 0 and s["stats"]["two_diff"] > 0
    p = len(case.reads) // 2 - 1
    q = order.tolist().index(p)
    assert s["bases"][300 * q:300 * q + 300] == "".join(case.reads[2 * p:2 * p + 2]).encode()
