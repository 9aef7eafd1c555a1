"""The device's own chain over tests/chain_cases.py's noisy construction, every step against its host model on the device's
own previous outputs, byte for byte and field for field:

  index_contigs -> align_reads -> align_gapped -> pair_inserts / aln_depths -> local_assm
                                              -> ctg_links -> scaffolds -> close_gaps -> select_contigs / fasta_text -> fasta_to_block
                                              -> shuffle_reads -> ctg_links again

The chain runs once, on device tensors, in a module-scoped fixture; each step takes the arrays the step before it returned.
A model's result is never replaced by a second device run.  What fails here and in no stage's own file lies in what one
stage hands the next on noisy data: clipped records of kind DP, reads with several records, repeated seeds, chimeric pairs,
rejected overlaps, disputed consensus columns (tests/test_chain_model.py asserts that the seed holds them all).  The
variants of a step run on the first SUBSET pairs where the full set adds nothing but model time.

The ground-truth claims of tests/test_chain_model.py are asserted again on the device's results: they do not rest on
the models."""
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
import mhm2_kmer_analysis_v2_amd as pkg
import scaffold_model as SM
import shuffle_model as SH
import unitig_model as UM
from test_chain_model import SEEDS
from test_gpu_gap_align import block_arrays, read_arrays

pytestmark = pytest.mark.gpu

K = CC.K
SUBSET = 100  # pairs of the variant passes
RECORDS = {"alns": A.ALN_DTYPE, "gapped": GM.GAP_ALN_DTYPE, "pairs": D.PAIR_DTYPE, "ctgs": D.CTG_DEPTH_DTYPE, "ends": LM.LASSM_END_DTYPE,
           "links": KM.LINK_DTYPE, "scafs": SM.SCAFFOLD_DTYPE, "members": SM.MEMBER_DTYPE, "closures": CM.CLOSURE_DTYPE}


def dev(a):
    """a host array as the device tensor the wrappers take: records as bytes, 64- and 16-bit unsigned as the signed type"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        a = np.frombuffer(a.tobytes(), dtype=np.uint8)
    elif a.dtype in (np.uint64, np.uint32, np.uint16):
        a = a.view({8: np.int64, 4: np.int32, 2: np.int16}[a.dtype.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype=None):
    """a device tensor (or host array) as a host array of dtype"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a if dtype is None else a.view(dtype)


def same_records(got, want, what):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        diff = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
        raise AssertionError("%s: %d records differ, the first at %d: device %s, model %s" % (what, len(diff), diff[0], got[diff[0]], want[diff[0]]))


def strings_of(seqs, offsets):
    text = bytes(bytearray(seqs)).decode()
    return [text[int(offsets[i]):int(offsets[i + 1]) - 1] for i in range(len(offsets) - 1)]


class Inputs:
    """the reads and the contig block of a case as host arrays, with on(side) giving them as the wrappers take them"""

    def __init__(self, case):
        self.case = case
        self.bases, self.offsets = read_arrays(case.reads)
        self.quals = np.frombuffer("".join(case.quals).encode(), dtype=np.uint8).copy()
        self.seqs, self.ctg_offsets = block_arrays(case.contigs)

    def on(self, device):
        f = dev if device else (lambda a: a)
        return f(self.bases), f(self.quals), f(self.offsets), f(self.seqs), f(self.ctg_offsets)


def run_chain(kc, inp, device):
    """the whole chain through the wrappers; every step's result as the wrapper returned it (R) and as host arrays (H)"""
    b, q, o, seqs, coffs = inp.on(device)
    R = {}
    R["index"] = kc.index_contigs(seqs, coffs)
    R["alns"], R["first"], R["align_st"] = kc.align_reads(b, o)
    R["gapped"], R["gap_st"] = kc.align_gapped(b, o, R["alns"])
    R["hist"], R["pairs"], R["insert_st"] = kc.pair_inserts(o, R["gapped"], max_insert=CC.MAX_INSERT)
    R["depths"], R["ctgs"], R["depth_st"] = kc.aln_depths(R["gapped"])
    R["lassm_seqs"], R["lassm_offsets"], R["ends"], R["lassm_st"] = kc.local_assm(b, q, o, R["gapped"], R["pairs"], ctg_depths=R["ctgs"], max_insert=CC.MAX_INSERT)
    R["links"], R["end_first"], R["link_st"], R["gap"] = kc.ctg_links(o, R["gapped"], R["pairs"], **CC.LINK_KW)
    R["scaf_seqs"], R["scaf_offsets"], R["scafs"], R["members"], R["scaf_st"] = kc.scaffolds(R["links"])
    (R["closed_seqs"], R["closed_offsets"], R["closed_scafs"], R["closed_members"], R["closures"],
     R["close_st"]) = kc.close_gaps(b, o, R["gapped"], R["scafs"], R["members"], **CC.CLOSE_KW)
    R["shuffled"] = kc.shuffle_reads(b, q, o, R["gapped"], R["pairs"], parts=3)
    R["order"], R["asm_st"] = kc.select_contigs(R["closed_seqs"], R["closed_offsets"], min_len=500, by_length=True)
    R["fasta"] = kc.fasta_text(R["closed_seqs"], R["closed_offsets"], line_width=60)
    H = {}
    for name, v in R.items():
        if name == "shuffled":
            H[name] = {k: (x if k == "stats" else host(x, {"gap_alns": GM.GAP_ALN_DTYPE, "pairs": D.PAIR_DTYPE, "order": np.uint32, "home": np.uint32,
                                                          "offsets": np.uint64, "part_starts": np.uint64}.get(k))) for k, x in v.items()}
        elif isinstance(v, (dict, bytes)) or name == "gap":
            H[name] = v
        else:
            rec = RECORDS.get(name, RECORDS.get(name.replace("closed_", "")))
            a = host(v)
            H[name] = a.view(rec) if rec else a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32, np.dtype(np.int16): np.uint16}.get(a.dtype, a.dtype))
    return R, H


class Run:
    pass


@pytest.fixture(scope="module", params=SEEDS)
def run(request):
    """the case, the device's chain on device tensors (R: the tensors, H: host copies) and the counter with the contigs' index"""
    import torch
    r = Run()
    r.case = CC.noisy_assembly(request.param)
    r.inp = Inputs(r.case)
    with pkg.KmerCounter(K) as kc:
        r.kc = kc
        r.R, r.H = run_chain(kc, r.inp, True)
        assert all(x.is_cuda for x in r.R.values() if isinstance(x, torch.Tensor))
        r.sub = r.case.subset(SUBSET)
        r.n_sub = int(r.H["first"][2 * SUBSET])  # the subset's align_reads records: the first ones
        yield r


# ---- every step against its model -------------------------------------------------------------------------------------
def test_index_and_align_reads(run):
    c, H = run.case, run.H
    index = A.Index(*A.join_block(c.contigs), K)
    assert H["index"] == index.stats and index.stats["repeated"] > 0
    b, _, o, _, _ = run.inp.on(True)
    for space in (1, 4):
        want = A.align_reads(index, c.reads, seed_space=space)
        got = (H["alns"], H["first"], H["align_st"]) if space == 1 else run.kc.align_reads(b, o, seed_space=4)
        same_records(host(got[0], A.ALN_DTYPE), want[0], "align_reads at seed space %d" % space)
        assert (host(got[1], np.uint64) == want[1]).all() and got[2] == want[2]
        assert want[2]["repeated_hits"] > 0 and (np.diff(want[1].astype(np.int64)) > 1).sum() > 10


def test_align_gapped_at_pad_16(run):
    c, H = run.case, run.H
    want, st = GM.align_gapped(c.contigs, c.reads, H["alns"], pad=16)
    same_records(H["gapped"], want, "align_gapped")
    assert H["gap_st"] == st and st["dp"] > 0 and st["exact"] > 0
    checked, skipped = CC.check_gapped(c, H["gapped"])
    assert checked > 600


def test_align_gapped_at_pad_64_on_the_subset(run):
    s, n = run.sub, run.n_sub
    b, _, o, _, _ = run.inp.on(True)
    got, st = run.kc.align_gapped(b[:int(run.inp.offsets[2 * SUBSET])], o[:2 * SUBSET + 1], run.R["alns"][:32 * n], pad=64)
    want, wst = GM.align_gapped(s.contigs, s.reads, run.H["alns"][:n], pad=64)
    same_records(host(got, GM.GAP_ALN_DTYPE), want, "align_gapped at pad 64")
    assert st == wst and wst["dp"] > 50


def test_pair_inserts(run):
    c, H = run.case, run.H
    hist, pairs, st = D.pair_inserts(c.ctg_lens, c.read_lens, H["gapped"], max_insert=CC.MAX_INSERT)
    same_records(H["pairs"], pairs, "pair_inserts")
    got_st = {k: v for k, v in H["insert_st"].items() if k not in ("mean", "stddev")}
    assert (H["hist"] == hist).all() and got_st == st and sum(1 for x in st["cls"] if x) >= 3


@pytest.mark.parametrize("per_contig", (False, True))
@pytest.mark.parametrize("best_only", (False, True))
def test_aln_depths(run, best_only, per_contig):
    c, H = run.case, run.H
    n = len(c.reads)
    for clip in (0, K):
        flags = (D.BEST_ONLY if best_only else 0) | (D.PER_CONTIG if per_contig else 0)
        want = D.aln_depths(c.ctg_lens, H["gapped"], edge_clip=clip, flags=flags, nreads=n if best_only else 0)
        if (best_only, per_contig, clip) == (False, False, 0):
            got = (H["depths"], H["ctgs"], H["depth_st"])
        else:
            got = run.kc.aln_depths(run.R["gapped"], edge_clip=clip, best_only=best_only, per_contig=per_contig, nreads=n if best_only else None)
        assert (host(got[0], np.uint16) == want[0]).all(), (clip, np.nonzero(host(got[0], np.uint16) != want[0])[0][:8])
        same_records(host(got[1], D.CTG_DEPTH_DTYPE), want[1], "aln_depths' contigs")
        assert got[2] == want[2] and (want[2]["not_best"] > 0) == best_only


def test_local_assm_with_the_devices_depths(run):
    c, H = run.case, run.H
    want = LM.local_assm(c.contigs, c.reads, c.quals, H["gapped"], H["pairs"], H["ctgs"]["mean"], k=K, max_insert=CC.MAX_INSERT)
    assert H["lassm_seqs"].tobytes() == want[0] and (H["lassm_offsets"] == want[1]).all()
    same_records(H["ends"], want[2], "local_assm's ends")
    assert H["lassm_st"] == want[3] and sum(1 for x in want[3]["status"] if x) >= 2
    assert CC.check_local_assm(c, H["lassm_seqs"], H["lassm_offsets"], H["ends"]) >= len(c.contigs)


LASSM_VARIANTS = {"no_depths": (False, {}), "permille_400": (True, dict(viable_permille=400)), "walks_of_60": (True, dict(max_walk_len=60))}


@pytest.mark.parametrize("name", sorted(LASSM_VARIANTS))
def test_local_assm_variants(run, name):
    """without depths; at a threshold the contig depths decide (400 thousandths of a mean of about 10 is over min_viable); with
    walks that end at their length"""
    c, H = run.case, run.H
    depths, kw = LASSM_VARIANTS[name]
    b, q, o, _, _ = run.inp.on(True)
    got = run.kc.local_assm(b, q, o, run.R["gapped"], run.R["pairs"], ctg_depths=run.R["ctgs"] if depths else None, max_insert=CC.MAX_INSERT, **kw)
    want = LM.local_assm(c.contigs, c.reads, c.quals, H["gapped"], H["pairs"], H["ctgs"]["mean"] if depths else None, k=K, max_insert=CC.MAX_INSERT, **kw)
    assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all()
    same_records(host(got[2], LM.LASSM_END_DTYPE), want[2], "local_assm's ends, " + name)
    assert got[3] == want[3]
    if name == "permille_400":
        assert 0 < want[3]["ext_bases"] < H["lassm_st"]["ext_bases"]
    if name == "walks_of_60":
        assert want[3]["status"][LM.MAX_LEN] > 0


@pytest.mark.parametrize("end_slack", (5, 0))
def test_ctg_links(run, end_slack):
    c, H = run.case, run.H
    kw = dict(CC.LINK_KW, end_slack=end_slack)
    want = KM.ctg_links(c.ctg_lens, c.read_lens, H["gapped"], H["pairs"], **kw)
    _, _, o, _, _ = run.inp.on(True)
    got = (H["links"], H["end_first"], H["link_st"], H["gap"]) if end_slack == 5 else run.kc.ctg_links(o, run.R["gapped"], run.R["pairs"], **kw)
    same_records(host(got[0], KM.LINK_DTYPE), want[0], "ctg_links at end_slack %d" % end_slack)
    assert (host(got[1], np.uint64) == want[1]).all() and got[2] == want[2] and (got[3] == KM.mean_gap(want[0])).all()
    assert want[2]["links_both"] > 0 and (end_slack == 0 or want[2]["spans_too_far"] > 0)
    checked, _ = CC.check_links(c, host(got[0], KM.LINK_DTYPE))
    assert checked >= len(c.gaps) // 2


@pytest.mark.parametrize("kw", ({}, dict(min_spans=1, max_second_permille=300), dict(overlap_slack=2)), ids=("defaults", "one_span_permille_300", "overlap_slack_2"))
def test_scaffolds(run, kw):
    c, H = run.case, run.H
    want = SM.scaffold(c.contigs, H["links"].view(SM.LINK_DTYPE), **kw)
    got = [H[n] for n in ("scaf_seqs", "scaf_offsets", "scafs", "members", "scaf_st")] if not kw else run.kc.scaffolds(run.R["links"], **kw)
    assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all()
    same_records(host(got[2], SM.SCAFFOLD_DTYPE), want[2], "scaffolds")
    same_records(host(got[3], SM.MEMBER_DTYPE), want[3], "scaffolds' members")
    assert got[4] == want[5]
    if not kw:
        assert want[5]["overlaps_checked"] > want[5]["overlaps_rejected"] > 0 and want[5]["scaffolds"] >= 2
        assert any(int(m["orient"]) for m in want[3]) and not all(int(m["orient"]) for m in want[3])


def test_close_gaps(run):
    c, H = run.case, run.H
    want = CM.close_gaps(c.contigs, c.reads, H["gapped"], H["scafs"].view(SM.SCAFFOLD_DTYPE), H["members"].view(SM.MEMBER_DTYPE), **CC.CLOSE_KW)
    assert H["closed_seqs"].tobytes() == want[0] and (H["closed_offsets"] == want[1]).all()
    for name, w in (("closed_scafs", want[2]), ("closed_members", want[3]), ("closures", want[4])):
        same_records(H[name], w, name)
    assert H["close_st"] == want[5] and want[5]["cands_off_join"] > 0 and want[5]["disputed_cols"] > 0 and want[5]["filled"] > 0
    CC.check_closed(c, strings_of(H["closed_seqs"], H["closed_offsets"]), H["close_st"])


def test_filters_and_caps_on_the_real_records(run):
    """the chain's own calls filter nothing and cap nothing; here the real scores and lengths meet min_score and min_len, and the
    reads with three records max_read_alns = 2"""
    c, H, R = run.case, run.H, run.R
    b, _, o, _, _ = run.inp.on(True)
    n, F = len(c.reads), dict(min_score=200, min_len=100)
    hist, pairs, ist = run.kc.pair_inserts(o, R["gapped"], max_insert=CC.MAX_INSERT, **F)
    wh, wp, wist = D.pair_inserts(c.ctg_lens, c.read_lens, H["gapped"], max_insert=CC.MAX_INSERT, **F)
    same_records(host(pairs, D.PAIR_DTYPE), wp, "pair_inserts with filters")
    assert (host(hist, np.uint64) == wh).all() and {k: v for k, v in ist.items() if k not in ("mean", "stddev")} == wist
    assert wist["reads_with_best"] < H["insert_st"]["reads_with_best"]
    got = run.kc.aln_depths(R["gapped"], edge_clip=K, best_only=True, nreads=n, **F)
    want = D.aln_depths(c.ctg_lens, H["gapped"], edge_clip=K, flags=D.BEST_ONLY, nreads=n, **F)
    assert (host(got[0], np.uint16) == want[0]).all() and got[2] == want[2] and want[2]["filtered"] > 0 and want[2]["not_best"] > 0
    same_records(host(got[1], D.CTG_DEPTH_DTYPE), want[1], "aln_depths with filters")
    for kw, pr, wpr in ((dict(CC.LINK_KW, **F), pairs, wp), (dict(CC.LINK_KW, max_read_alns=2), R["pairs"], H["pairs"])):
        links, end_first, st, _ = run.kc.ctg_links(o, R["gapped"], pr, **kw)
        w = KM.ctg_links(c.ctg_lens, c.read_lens, H["gapped"], wpr, **kw)
        same_records(host(links, KM.LINK_DTYPE), w[0], "ctg_links with %s" % sorted(set(kw) - set(CC.LINK_KW)))
        assert (host(end_first, np.uint64) == w[1]).all() and st == w[2] and (w[2]["filtered"] > 0 or w[2]["reads_over_cap"] > 0)
    kw = dict(CC.CLOSE_KW, max_read_alns=2, min_score=60, min_len=30)
    got = run.kc.close_gaps(b, o, R["gapped"], R["scafs"], R["members"], **kw)
    want = CM.close_gaps(c.contigs, c.reads, H["gapped"], H["scafs"].view(SM.SCAFFOLD_DTYPE), H["members"].view(SM.MEMBER_DTYPE), **kw)
    assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all()
    for g, w, dt in zip(got[2:5], want[2:5], (SM.SCAFFOLD_DTYPE, SM.MEMBER_DTYPE, CM.CLOSURE_DTYPE)):
        same_records(host(g, dt), w, "close_gaps with a cap and filters")
    assert got[5] == want[5] and want[5]["reads_over_cap"] > 0 and want[5]["passed"] < H["close_st"]["passed"]


def test_align_variants_on_the_real_reads(run):
    """align_reads with a mismatch bound, and align_gapped with every record through the dynamic programme under the
    alternate scores at pad 0 (the subset)"""
    c, H = run.case, run.H
    b, _, o, _, _ = run.inp.on(True)
    index = A.Index(*A.join_block(c.contigs), K)
    alns, first, st = run.kc.align_reads(b, o, max_mismatches=2)
    want = A.align_reads(index, c.reads, max_mismatches=2)
    same_records(host(alns, A.ALN_DTYPE), want[0], "align_reads with at most two mismatches")
    assert (host(first, np.uint64) == want[1]).all() and st == want[2] and 0 < want[2]["alignments"] < H["align_st"]["alignments"]
    s, n = run.sub, run.n_sub
    got, gst = run.kc.align_gapped(b[:int(run.inp.offsets[2 * SUBSET])], o[:2 * SUBSET + 1], run.R["alns"][:32 * n], pad=0, scores=GM.SCORES_ALTERNATE,
                                   always_dp=True)
    wg, wst = GM.align_gapped(s.contigs, s.reads, H["alns"][:n], pad=0, scores=GM.SCORES_ALTERNATE, always_dp=True)
    same_records(host(got, GM.GAP_ALN_DTYPE), wg, "align_gapped, always the dynamic programme")
    assert gst == wst and wst["exact"] == 0


def test_shuffle_reads_and_the_links_behind_it(run):
    c, H, inp = run.case, run.H, run.inp
    s, S = run.R["shuffled"], H["shuffled"]
    want = SH.shuffle_reads(c.ctg_lens, inp.bases.tobytes(), inp.quals.tobytes(), inp.offsets, H["gapped"], H["pairs"], 3)
    for k in ("bases", "quals", "offsets", "order", "home", "part_starts", "gap_alns", "pairs"):
        assert S[k].tobytes() == want[k], k
    assert S["stats"] == want["stats"] and S["stats"]["two_diff"] > 0 and S["stats"]["one_mate"] > 0
    order = S["order"].tolist()
    assert sorted(order) == list(range(len(c.reads) // 2)) and order != sorted(order)
    # what it hands back goes through ctg_links again: the model's links on the shuffled set are the device's, and the old ones
    links, end_first, st, _ = run.kc.ctg_links(s["offsets"], s["gap_alns"], s["pairs"], **CC.LINK_KW)
    read_lens = np.diff(S["offsets"].astype(np.int64)).tolist()
    w = KM.ctg_links(c.ctg_lens, read_lens, S["gap_alns"], S["pairs"], **CC.LINK_KW)
    same_records(host(links, KM.LINK_DTYPE), w[0], "ctg_links on the shuffled reads")
    assert (host(end_first, np.uint64) == w[1]).all() and st == w[2]
    assert w[0].tobytes() == H["links"].tobytes() and st == H["link_st"]


def test_selection_fasta_text_and_the_way_back(run):
    H, R = run.H, run.R
    order, st = AM.select(H["closed_seqs"], H["closed_offsets"], 500, True)
    assert H["order"].tolist() == order and H["asm_st"] == st and st["selected"] >= 2 and st["n"] == 0
    text = AM.fasta(H["closed_seqs"], H["closed_offsets"], None, "scaffold_", 60)
    assert H["fasta"] == text
    cut = len(text) // 3 + 7  # two windows: inside a line
    windows = [run.kc.fasta_text(R["closed_seqs"], R["closed_offsets"], line_width=60, first_byte=f, capacity=n) for f, n in ((0, cut), (cut, None))]
    assert windows == [AM.window(text, 0, cut), AM.window(text, cut, len(text))] and b"".join(windows) == text
    selected = run.kc.fasta_text(R["closed_seqs"], R["closed_offsets"], R["order"], line_width=60)
    assert selected == AM.fasta(H["closed_seqs"], H["closed_offsets"], order, "scaffold_", 60)
    back = run.kc.fasta_to_block(dev(np.frombuffer(text, dtype=np.uint8)))
    want = FM.parse(text)
    assert back["seqs"].is_cuda and host(back["seqs"]).tobytes() == want["seqs"].tobytes() and (host(back["offsets"], np.uint64) == want["offsets"]).all()
    assert host(back["records"], FM.REC_DTYPE).tobytes() == want["records"].tobytes() and back["stats"] == want["stats"]
    # the block read back is the block written
    assert host(back["seqs"]).tobytes() == H["closed_seqs"].tobytes() and (host(back["offsets"], np.uint64) == H["closed_offsets"]).all()


@pytest.mark.parametrize("which", ("lassm", "scaf", "closed"))
def test_second_round_on_the_devices_own_blocks(run, which):
    """the block a kernel wrote on noisy data (the extended contigs, the scaffolds with their N runs, the closed scaffolds)
    becomes the input of the index: device against model, on the device's block"""
    c, H, R = run.case, run.H, run.R
    b, _, o, _, _ = run.inp.on(True)
    contigs = strings_of(H[which + "_seqs"], H[which + "_offsets"])
    index = A.Index(*A.join_block(contigs), K)
    want = A.align_reads(index, c.reads)
    with pkg.KmerCounter(K) as kc:  # a counter of its own: the fixture's keeps the contigs' index
        assert kc.index_contigs(R[which + "_seqs"], R[which + "_offsets"]) == index.stats
        alns, first, st = kc.align_reads(b, o)
        same_records(host(alns, A.ALN_DTYPE), want[0], "align_reads on the %s block" % which)
        assert (host(first, np.uint64) == want[1]).all() and st == want[2]
        n = int(want[1][2 * SUBSET])
        gapped, gst = kc.align_gapped(b[:int(run.inp.offsets[2 * SUBSET])], o[:2 * SUBSET + 1], alns[:32 * n])
        wg, wst = GM.align_gapped(contigs, c.reads[:2 * SUBSET], want[0][:n])
        same_records(host(gapped, GM.GAP_ALN_DTYPE), wg, "align_gapped on the %s block" % which)
        assert gst == wst
    if which == "scaf":
        assert index.stats["bases"] > index.stats["windows"] + (K - 1) * len(contigs)  # N runs: windows that are no seeds


def test_host_arrays_give_the_same_bytes(run):
    with pkg.KmerCounter(K) as kc:
        R, H = run_chain(kc, run.inp, False)
    assert all(isinstance(x, np.ndarray) for x in R.values() if not isinstance(x, (dict, bytes)))
    for name, want in run.H.items():
        if name == "shuffled":
            for k, w in want.items():
                assert (H[name][k] == w) if k == "stats" else (H[name][k].tobytes() == w.tobytes()), k
        elif isinstance(want, (dict, bytes)):
            assert H[name] == want, name
        else:
            assert H[name].tobytes() == want.tobytes(), name


# ---- from the reads alone: the contigs are the device's own unitigs ---------------------------------------------------------
def test_from_the_reads_alone_through_the_devices_unitigs(run):
    """submit_reads at k = 21 -> unitig_block / index_unitigs -> the chain through local_assm and scaffolds, the SUBSET pairs aligned.  Only
    model equality: with errors the unitigs are many and short, and no ground truth is claimed."""
    c, inp, s = run.case, run.inp, run.sub
    b, q, o, _, _ = inp.on(True)
    nb = int(inp.offsets[2 * SUBSET])
    sb, so = b[:nb], o[:2 * SUBSET + 1]
    with pkg.KmerCounter(K) as kc:
        kc.submit_reads(b, q, o)
        kc.flush()
        keys, counts, left, right = kc.results()
        units, ust = UM.unitigs(UM.results_dict(keys, counts, left, right, K), K)
        w_seqs, w_depths, w_offsets, _ = UM.block(units)
        seqs, depths = kc.unitig_block()
        assert host(seqs).tobytes() == w_seqs and (host(depths, np.uint16) == w_depths).all() and ust["unitigs"] > 10
        contigs = [u[0] for u in units]
        lens = [len(x) for x in contigs]
        index = A.Index(*A.join_block(contigs), K)
        assert kc.index_unitigs() == index.stats and kc.contig_index_info() == (len(w_seqs), len(units))
        alns, first, ast = kc.align_reads(sb, so)
        want = A.align_reads(index, s.reads)
        same_records(host(alns, A.ALN_DTYPE), want[0], "align_reads on the unitigs")
        assert (host(first, np.uint64) == want[1]).all() and ast == want[2]
        gapped, gst = kc.align_gapped(sb, so, alns)
        wg, wgst = GM.align_gapped(contigs, s.reads, want[0])
        same_records(host(gapped, GM.GAP_ALN_DTYPE), wg, "align_gapped on the unitigs")
        assert gst == wgst
        hist, pairs, ist = kc.pair_inserts(so, gapped, max_insert=CC.MAX_INSERT)
        wh, wp, wist = D.pair_inserts(lens, s.read_lens, wg, max_insert=CC.MAX_INSERT)
        same_records(host(pairs, D.PAIR_DTYPE), wp, "pair_inserts on the unitigs")
        assert (host(hist, np.uint64) == wh).all() and {k: v for k, v in ist.items() if k not in ("mean", "stddev")} == wist
        depths, ctgs, dst = kc.aln_depths(gapped)
        wd = D.aln_depths(lens, wg)
        same_records(host(ctgs, D.CTG_DEPTH_DTYPE), wd[1], "aln_depths on the unitigs")
        assert (host(depths, np.uint16) == wd[0]).all() and dst == wd[2]
        got = kc.local_assm(sb, q[:nb], so, gapped, pairs, ctg_depths=ctgs, max_insert=CC.MAX_INSERT)
        wa = LM.local_assm(contigs, s.reads, s.quals, wg, wp, wd[1]["mean"], k=K, max_insert=CC.MAX_INSERT)
        assert host(got[0]).tobytes() == wa[0] and (host(got[1], np.uint64) == wa[1]).all() and got[3] == wa[3]
        same_records(host(got[2], LM.LASSM_END_DTYPE), wa[2], "local_assm on the unitigs")
        links, end_first, lst, _ = kc.ctg_links(so, gapped, pairs, **CC.LINK_KW)
        wl = KM.ctg_links(lens, s.read_lens, wg, wp, **CC.LINK_KW)
        same_records(host(links, KM.LINK_DTYPE), wl[0], "ctg_links on the unitigs")
        assert (host(end_first, np.uint64) == wl[1]).all() and lst == wl[2]
        got = kc.scaffolds(links, min_spans=1)
        ws = SM.scaffold(contigs, wl[0], min_spans=1)
        assert host(got[0]).tobytes() == ws[0] and (host(got[1], np.uint64) == ws[1]).all()
        same_records(host(got[2], SM.SCAFFOLD_DTYPE), ws[2], "scaffolds of the unitigs")
        same_records(host(got[3], SM.MEMBER_DTYPE), ws[3], "members of the unitigs' scaffolds")
        assert got[4] == ws[5]
