"""The contig pass on memory that is not zero when the library gets it: KC_DEBUG_FILL fills every fresh allocation of the
library ("Poisoned scratch"), 0xA5 and 0x5A a case, and every step still equals its host model exactly.  The case
is tests/chain_cases.py's noisy construction on its first 100 pairs (SUBSET); the models run once, as a chain
(test_chain_model.model_chain, about a second), and every step's device call takes the MODEL's hand-over, so that a step's
test does not wait for the others and a wrong step does not hide behind the one before it.  Device tensors and host arrays
alike: a host caller's arrays are staged in the call's own scratch, which is filled too.  Contexts are made after the
variable is set, and every test checks that kc_debug_filled_bytes() rose.

Beside the ordinary case every step runs where some or all of its items write nothing: no reads at all; reads of which
none has a record (every pair of class NONE, every read without a slot, every contig untouched, every end without a
candidate, zero runs of links, every pair homeless); links that no filter passes; scaffolds without a gap (every contig
its own scaffold); more parts than pairs.  The size queries and the second calls with the size the first reported run
at the ABI as well (early_exits): behind the wrapper's full call of kc_align_reads, kc_local_assm, kc_ctg_links, kc_scaffold,
kc_close_gaps, kc_ctg_dedup and kc_fasta_text -- in the ordinary case and in the cases where items write nothing -- the
same arguments go in again with every output NULL, and with the one bounded array an item short; totals, statistics and
status must be the full call's, and one short nothing is written.  (kc_align_gapped has neither form: its one output has
as many records as its input and NULL is KC_ERR_INVALID_ARG; kc_fasta_text's capacity is a window, one short is a prefix.)  Wall time on the MI355X: 4 s for the module's 32 tests."""
import ctypes as C

import numpy as np
import pytest

import align_model as A
import asm_model as AM
import chain_cases as CC
import close_model as CM
import dedup_model as DM
import depth_model as D
import gap_model as GM
import lassm_model as LM
import links_model as KM
import mhm2_kmer_analysis_v2_amd as pkg
import scaffold_model as SM
import shuffle_model as SH
from mhm2_kmer_analysis_v2_amd import _lib
from mhm2_kmer_analysis_v2_amd.kcount import _stats_dict as kcount_stats
from test_chain_model import SEEDS, model_chain
from test_gpu_chain_noisy import SUBSET, Inputs, dev, host, same_records

pytestmark = pytest.mark.gpu

K = CC.K
FILLS = (0xA5, 0x5A)
SIDES = pytest.mark.parametrize("device", (True, False), ids=("device", "host"))


@pytest.fixture(params=FILLS, ids=["0xA5", "0x5A"])
def fill(request, monkeypatch):
    monkeypatch.setenv("KC_DEBUG_FILL", "0x%02X" % request.param)
    before = pkg.lib().kc_debug_filled_bytes()
    yield request.param
    assert pkg.lib().kc_debug_filled_bytes() > before, "nothing was filled: the test proves nothing"


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class Chain:
    """the case, its arrays, and every model's result on the result of the model before it"""

    def __init__(self):
        self.case = CC.noisy_assembly(SEEDS[0]).subset(SUBSET)
        self.inp = Inputs(self.case)
        self.out, _ = model_chain(self.case)
        o = self.out
        self.alns, self.first, self.align_st = o["align"]
        self.gapped, self.gap_st = o["gapped"]
        self.hist, self.pairs, self.insert_st = o["pairs"]
        self.depths, self.ctgs, self.depth_st = o["depths"]
        self.links = o["links"][0]
        self.scafs, self.members = o["scaffolds"][2], o["scaffolds"][3]
        self.no_alns = self.gapped[:0]
        self.no_pairs = D.pair_inserts(self.case.ctg_lens, self.case.read_lens, self.no_alns, max_insert=CC.MAX_INSERT)[1]


def chain():
    return cached("chain", Chain)


def side(device, *arrays):
    return tuple(dev(a) if device else a for a in arrays)


class Ctx:
    """a counter with the case's contigs indexed, and the reads on the side asked for"""

    def __init__(self, device):
        c = chain()
        self.kc = pkg.KmerCounter(K)
        self.b, self.q, self.o, seqs, coffs = c.inp.on(device)
        self.index = self.kc.index_contigs(seqs, coffs)
        self.no_b, self.no_o = side(device, c.inp.bases[:0], c.inp.offsets[:1])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.kc.close()


class Spy:
    """the library as kcount.py sees it, with the arguments and the status of every entry point's last call kept"""

    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        f = getattr(self.real, name)

        def call(*args):
            rc = f(*args)
            self.calls[name] = (args, rc)
            return rc
        return call


@pytest.fixture
def spy(monkeypatch):
    from mhm2_kmer_analysis_v2_amd import kcount
    s = Spy(pkg.lib())
    monkeypatch.setattr(kcount, "lib", lambda: s)
    return s


CANARY = 0xC3


def early_exits(spy, name, device, outs, cap, totals, stats, item=1, bound=None):
    """The two calls of an entry point that end early, made at the ABI with the arguments of the wrapper's last, full call of it
    (whose results the test holds against the model): a size query -- every output NULL, capacity 0 -- and a call whose one
    bounded array holds one item less than the call reported (the other outputs NULL: all are optional).  Either must report
    the full call's totals and statistics; the first is KC_OK, the second KC_ERR_CAPACITY with nothing written.  outs, cap,
    totals, stats: positions in the argument list; item: bytes of an item of the bounded array outs[0]; bound: the total the
    capacity is held against (by default the last)."""
    import torch
    args, rc = spy.calls[name]
    assert rc == _lib.KC_OK, name
    fn = getattr(spy.real, name)
    full_totals = [int(args[t]._obj.value) for t in totals]
    full_stats = kcount_stats(args[stats]._obj) if stats is not None else None

    def again(change):
        a = list(args)
        for o in outs:
            a[o] = None
        a[cap] = 0
        fresh = [C.c_uint64(0xDEAD) for _ in totals]
        for t, v in zip(totals, fresh):
            a[t] = C.byref(v)
        st = type(args[stats]._obj)() if stats is not None else None
        if st is not None:
            a[stats] = C.byref(st)
        change(a)
        rc = fn(*a)
        assert [int(v.value) for v in fresh] == full_totals, (name, rc, [int(v.value) for v in fresh], full_totals)
        assert st is None or kcount_stats(st) == full_stats, (name, rc)
        return rc
    assert again(lambda a: None) == _lib.KC_OK, name + ": the size query"
    n = full_totals[totals.index(bound)] if bound is not None else full_totals[-1]
    if n == 0:
        return
    room = torch.full(((n - 1) * item + 64,), CANARY, dtype=torch.uint8, device="cuda") if device else np.full((n - 1) * item + 64, CANARY, dtype=np.uint8)

    def short(a):
        a[outs[0]] = room.data_ptr() if device else room.ctypes.data
        a[cap] = n - 1
    assert again(short) == _lib.KC_ERR_CAPACITY, name + ": capacity one short"
    assert bool((room == CANARY).all()), name + ": one short, and something was written"


@SIDES
def test_index_and_align_reads(fill, spy, device):
    c = chain()
    with Ctx(device) as x:
        assert x.index == c.out["index"].stats
        for seed_space in (1, 4):
            want = cached(("align", seed_space), lambda: A.align_reads(c.out["index"], c.case.reads, seed_space=seed_space))
            alns, first, st = x.kc.align_reads(x.b, x.o, seed_space=seed_space)
            early_exits(spy, "kc_align_reads", device, outs=(7, 9), cap=8, totals=(10,), stats=11, item=32)
            same_records(host(alns, A.ALN_DTYPE), want[0], "align_reads")
            assert (host(first, np.uint64) == want[1]).all() and st == want[2]
        alns, first, st = x.kc.align_reads(x.no_b, x.no_o)  # no reads
        assert len(host(alns)) == 0 and host(first, np.uint64).tolist() == [0] and st["reads"] == 0 and st["alignments"] == 0
        # reads too short to hold a seed: every read writes a count of 0
        short = ["ACGT" * 4] * 70
        sb, so = side(device, np.frombuffer("".join(short).encode(), dtype=np.uint8), np.arange(71, dtype=np.uint64) * 16)
        alns, first, st = x.kc.align_reads(sb, so)
        assert len(host(alns)) == 0 and (host(first, np.uint64) == 0).all() and st["reads"] == 70 and st["windows"] == 0


@SIDES
def test_align_gapped(fill, device):
    c = chain()
    with Ctx(device) as x:
        alns, = side(device, c.alns)
        got, st = x.kc.align_gapped(x.b, x.o, alns)
        same_records(host(got, GM.GAP_ALN_DTYPE), c.gapped, "align_gapped")
        assert st == c.gap_st and st["dp"] > 0 and st["exact"] > 0
        want = cached("gapped exact only", lambda: GM.align_gapped(c.case.contigs, c.case.reads, c.alns[c.gapped["kind"] == GM.KIND_EXACT]))
        exact, = side(device, np.ascontiguousarray(c.alns[c.gapped["kind"] == GM.KIND_EXACT]))
        got, st = x.kc.align_gapped(x.b, x.o, exact)  # nothing for the dynamic programme: an empty list
        same_records(host(got, GM.GAP_ALN_DTYPE), want[0], "align_gapped, exact records only")
        assert st == want[1] and st["dp"] == 0
        got, st = x.kc.align_gapped(x.b, x.o, side(device, c.alns[:0])[0])  # no records
        assert len(host(got)) == 0 and st["records"] == 0


@SIDES
def test_pair_inserts_and_aln_depths(fill, device):
    c = chain()
    n = len(c.case.reads)
    with Ctx(device) as x:
        gapped, none = side(device, c.gapped, c.no_alns)
        hist, pairs, st = x.kc.pair_inserts(x.o, gapped, max_insert=CC.MAX_INSERT)
        same_records(host(pairs, D.PAIR_DTYPE), c.pairs, "pair_inserts")
        assert (host(hist, np.uint64) == c.hist).all() and {k: v for k, v in st.items() if k not in ("mean", "stddev")} == c.insert_st
        want = cached("no pairs", lambda: D.pair_inserts(c.case.ctg_lens, c.case.read_lens, c.no_alns, max_insert=CC.MAX_INSERT))
        hist, pairs, st = x.kc.pair_inserts(x.o, none, max_insert=CC.MAX_INSERT)  # reads without a record: every pair of class NONE
        same_records(host(pairs, D.PAIR_DTYPE), want[1], "pair_inserts without records")
        assert (host(hist, np.uint64) == 0).all() and {k: v for k, v in st.items() if k not in ("mean", "stddev")} == want[2]
        hist, pairs, st = x.kc.pair_inserts(x.no_o, none, max_insert=CC.MAX_INSERT)  # no reads
        assert len(host(pairs)) == 0 and (host(hist, np.uint64) == 0).all() and st["pairs"] == 0
        for best_only, per_contig, clip in ((False, False, 0), (True, False, K), (False, True, 0), (True, True, K)):
            flags = (D.BEST_ONLY if best_only else 0) | (D.PER_CONTIG if per_contig else 0)
            for name, recs, d_recs in (("all", c.gapped, gapped), ("none", c.no_alns, none)):  # none: contigs that no read touches
                want = cached(("depths", flags, clip, name), lambda: D.aln_depths(c.case.ctg_lens, recs, edge_clip=clip, flags=flags, nreads=n if best_only else 0))
                got = x.kc.aln_depths(d_recs, edge_clip=clip, best_only=best_only, per_contig=per_contig, nreads=n if best_only else None)
                assert (host(got[0], np.uint16) == want[0]).all(), (flags, name)
                same_records(host(got[1], D.CTG_DEPTH_DTYPE), want[1], "aln_depths' contigs")
                assert got[2] == want[2]


@SIDES
def test_local_assm(fill, spy, device):
    c = chain()
    with Ctx(device) as x:
        gapped, pairs, ctgs, none, no_pairs = side(device, c.gapped, c.pairs, c.ctgs, c.no_alns, c.no_pairs)
        want = c.out["lassm"]
        got = x.kc.local_assm(x.b, x.q, x.o, gapped, pairs, ctg_depths=ctgs)
        early_exits(spy, "kc_local_assm", device, outs=(11, 13, 14), cap=12, totals=(15,), stats=16)
        assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all() and got[3] == want[3]
        same_records(host(got[2], LM.LASSM_END_DTYPE), want[2], "local_assm's ends")
        assert want[3]["ext_bases"] > 0
        # reads without a record: no end has a candidate, the block comes back as it is
        want = cached("lassm none", lambda: LM.local_assm(c.case.contigs, c.case.reads, c.case.quals, c.no_alns, c.no_pairs, None, k=K))
        got = x.kc.local_assm(x.b, x.q, x.o, none, no_pairs)
        early_exits(spy, "kc_local_assm", device, outs=(11, 13, 14), cap=12, totals=(15,), stats=16)
        assert host(got[0]).tobytes() == want[0] == c.inp.seqs.tobytes() and (host(got[1], np.uint64) == want[1]).all() and got[3] == want[3]
        same_records(host(got[2], LM.LASSM_END_DTYPE), want[2], "local_assm's ends without records")
        # walks that end at their length, and a cap of candidates that most ends are over
        for kw in (dict(max_walk_len=20), dict(max_cands=3)):
            want = cached(("lassm", str(kw)), lambda: LM.local_assm(c.case.contigs, c.case.reads, c.case.quals, c.gapped, c.pairs, c.ctgs["mean"], k=K, **kw))
            got = x.kc.local_assm(x.b, x.q, x.o, gapped, pairs, ctg_depths=ctgs, **kw)
            assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all() and got[3] == want[3], kw
            same_records(host(got[2], LM.LASSM_END_DTYPE), want[2], "local_assm's ends, %s" % kw)


@SIDES
def test_ctg_links_and_scaffolds(fill, spy, device):
    c = chain()
    with Ctx(device) as x:
        gapped, pairs, none, no_pairs = side(device, c.gapped, c.pairs, c.no_alns, c.no_pairs)
        want = c.out["links"]
        links, end_first, st, gap = x.kc.ctg_links(x.o, gapped, pairs, **CC.LINK_KW)
        early_exits(spy, "kc_ctg_links", device, outs=(8, 10), cap=9, totals=(11,), stats=12, item=48)
        same_records(host(links, KM.LINK_DTYPE), want[0], "ctg_links")
        assert (host(end_first, np.uint64) == want[1]).all() and st == want[2] and (gap == KM.mean_gap(want[0])).all() and st["links_both"] > 0
        # no record passes the filters (no read has a slot, the spans alone link); reads without a record and no reads: zero runs
        for name, recs, prs, d_recs, d_prs, offs, lens, kw in (
                ("filtered", c.gapped, c.pairs, gapped, pairs, x.o, c.case.read_lens, dict(CC.LINK_KW, min_score=100000)),
                ("no records", c.no_alns, c.no_pairs, none, no_pairs, x.o, c.case.read_lens, CC.LINK_KW),
                ("no reads", c.no_alns, c.no_pairs[:0], none, side(device, c.no_pairs[:0])[0], x.no_o, [], CC.LINK_KW)):
            w = cached(("links", name), lambda: KM.ctg_links(c.case.ctg_lens, lens, recs, prs, **kw))
            links, end_first, st, gap = x.kc.ctg_links(offs, d_recs, d_prs, **kw)
            early_exits(spy, "kc_ctg_links", device, outs=(8, 10), cap=9, totals=(11,), stats=12, item=48)
            same_records(host(links, KM.LINK_DTYPE), w[0], "ctg_links, " + name)
            assert (host(end_first, np.uint64) == w[1]).all() and st == w[2], name
            assert (name == "filtered" and st["passed"] == 0 and st["links_span_only"] == len(w[0]) // 2 > 0) or (len(w[0]) == 0 and (w[1] == 0).all()), name
        # the splints alone (no pairs): units are the reads only
        w = cached(("links", "splints"), lambda: KM.ctg_links(c.case.ctg_lens, c.case.read_lens, c.gapped, None, **CC.LINK_KW))
        links, end_first, st, gap = x.kc.ctg_links(x.o, gapped, None, **CC.LINK_KW)
        same_records(host(links, KM.LINK_DTYPE), w[0], "ctg_links without pairs")
        assert (host(end_first, np.uint64) == w[1]).all() and st == w[2]
        d_links, = side(device, c.links)
        for kw in ({}, dict(min_spans=1, max_second_permille=300), dict(min_splints=1000, min_spans=1000)):  # the last: no link qualifies
            want = cached(("scaffolds", str(kw)), lambda: SM.scaffold(c.case.contigs, c.links.view(SM.LINK_DTYPE), **kw))
            got = x.kc.scaffolds(d_links, **kw)
            early_exits(spy, "kc_scaffold", device, outs=(5, 7, 8, 9, 10), cap=6, totals=(11, 12), stats=13)
            assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all() and got[4] == want[5], kw
            same_records(host(got[2], SM.SCAFFOLD_DTYPE), want[2], "scaffolds")
            same_records(host(got[3], SM.MEMBER_DTYPE), want[3], "scaffolds' members")
        want = cached(("scaffolds", "no links"), lambda: SM.scaffold(c.case.contigs, c.links[:0].view(SM.LINK_DTYPE)))
        got = x.kc.scaffolds(side(device, c.links[:0])[0])  # no links: every contig its own scaffold, none with a gap
        assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all() and got[4] == want[5]
        assert want[5]["scaffolds"] == want[5]["singletons"] == len(c.case.contigs)
        same_records(host(got[2], SM.SCAFFOLD_DTYPE), want[2], "scaffolds without links")
        same_records(host(got[3], SM.MEMBER_DTYPE), want[3], "their members")


@SIDES
def test_close_gaps(fill, spy, device):
    c = chain()
    with Ctx(device) as x:
        gapped, scafs, members, none = side(device, c.gapped, c.scafs, c.members, c.no_alns)
        singles = cached(("scaffolds", "no links"), lambda: SM.scaffold(c.case.contigs, c.links[:0].view(SM.LINK_DTYPE)))
        s_scafs, s_members = side(device, singles[2], singles[3])
        for name, recs, d_recs, sc, mb, d_sc, d_mb, b, o, reads in (
                ("ordinary", c.gapped, gapped, c.scafs, c.members, scafs, members, x.b, x.o, c.case.reads),
                ("reads without a record", c.no_alns, none, c.scafs, c.members, scafs, members, x.b, x.o, c.case.reads),
                ("no reads", c.no_alns, none, c.scafs, c.members, scafs, members, x.no_b, x.no_o, []),
                ("scaffolds without gaps", c.gapped, gapped, singles[2], singles[3], s_scafs, s_members, x.b, x.o, c.case.reads)):
            want = cached(("closed", name), lambda: CM.close_gaps(c.case.contigs, reads, recs, sc.view(SM.SCAFFOLD_DTYPE), mb.view(SM.MEMBER_DTYPE), **CC.CLOSE_KW))
            got = x.kc.close_gaps(b, o, d_recs, d_sc, d_mb, **CC.CLOSE_KW)
            early_exits(spy, "kc_close_gaps", device, outs=(11, 13, 14, 15, 16), cap=12, totals=(17,), stats=18)
            assert host(got[0]).tobytes() == want[0] and (host(got[1], np.uint64) == want[1]).all() and got[5] == want[5], name
            for g, w, dt in zip(got[2:5], want[2:5], (SM.SCAFFOLD_DTYPE, SM.MEMBER_DTYPE, CM.CLOSURE_DTYPE)):
                same_records(host(g, dt), w, "close_gaps, " + name)
            if name == "ordinary":
                assert want[5]["filled"] > 0 and want[5]["cands_off_join"] > 0
            else:
                assert want[5]["filled"] == 0


@SIDES
def test_shuffle_reads(fill, device):
    c = chain()
    inp = c.inp
    with Ctx(device) as x:
        gapped, pairs, none, no_pairs = side(device, c.gapped, c.pairs, c.no_alns, c.no_pairs)
        for name, recs, prs, d_recs, d_prs, parts in (("three parts", c.gapped, c.pairs, gapped, pairs, 3), ("more parts than pairs", c.gapped, c.pairs, gapped, pairs, 250),
                                                      ("every pair homeless", c.no_alns, c.no_pairs, none, no_pairs, 3)):
            want = cached(("shuffled", name), lambda: SH.shuffle_reads(c.case.ctg_lens, inp.bases.tobytes(), inp.quals.tobytes(), inp.offsets, recs, prs, parts))
            got = x.kc.shuffle_reads(x.b, x.q, x.o, d_recs, d_prs, parts=parts)
            for k in ("bases", "quals", "offsets", "order", "home", "part_starts", "gap_alns", "pairs"):
                assert host(got[k]).tobytes() == want[k], (name, k)
            assert got["stats"] == want["stats"], name
        assert cached(("shuffled", "every pair homeless"), None)["stats"]["homeless"] == SUBSET
        want = cached(("shuffled", "no reads"), lambda: SH.shuffle_reads(c.case.ctg_lens, b"", b"", inp.offsets[:1], c.no_alns, c.no_pairs[:0], 3))
        got = x.kc.shuffle_reads(x.no_b, x.no_b, x.no_o, none, side(device, c.no_pairs[:0])[0], parts=3)
        for k in ("bases", "quals", "offsets", "order", "home", "part_starts"):
            assert host(got[k]).tobytes() == want[k], ("no reads", k)
        assert got["stats"] == want["stats"]


@SIDES
def test_selection_fasta_text_and_dedup(fill, spy, device):
    c = chain()
    seqs, offs = np.frombuffer(c.out["closed"][0], dtype=np.uint8), c.out["closed"][1]
    with pkg.KmerCounter(K) as kc:
        d_seqs, d_offs = side(device, seqs, offs)
        for min_len, by_length in ((500, True), (0, False), (100000, True)):  # the last: nothing is selected
            want = cached(("select", min_len, by_length), lambda: AM.select(seqs, offs, min_len, by_length))
            order, st = kc.select_contigs(d_seqs, d_offs, min_len=min_len, by_length=by_length)
            assert host(order, np.uint32).tolist() == want[0] and st == want[1], (min_len, by_length)
        order = cached(("select", 500, True), None)[0]
        for od, width in ((None, 60), (order, 60), (order[:1], 0), ([], 60)):
            want = cached(("fasta", str(od), width), lambda: AM.fasta(seqs, offs, od, "scaffold_", width))
            d_od = None if od is None else side(device, np.asarray(od, dtype=np.uint32))[0]
            assert kc.fasta_text(d_seqs, d_offs, d_od, line_width=width) == want, (od, width)
            if want:  # (the wrapper makes no call for an empty order)
                args, rc = spy.calls["kc_fasta_text"]
                a, written, total = list(args), C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
                a[10], a[11], a[12], a[13] = None, 1 << 20, C.byref(written), C.byref(total)
                assert spy.real.kc_fasta_text(*a) == _lib.KC_OK and (written.value, total.value) == (0, len(want))  # NULL text: a size query
                assert kc.fasta_text(d_seqs, d_offs, d_od, line_width=width, capacity=len(want) - 1) == want[:-1]
            cut = len(want) // 3 + 7
            if cut < len(want):
                assert kc.fasta_text(d_seqs, d_offs, d_od, line_width=width, first_byte=cut, capacity=len(want) - cut - 1) == want[cut:-1]
        # the case's contigs with a planted copy and a planted slice of a reverse complement; then a block without either
        ctgs = list(c.case.contigs)
        planted = ctgs + [ctgs[0], DM.rc(ctgs[1].encode())[10:150]]
        for name, cs, kw in (("planted", planted, {}), ("planted, two mismatches", planted, dict(max_mismatches=2)), ("nothing to remove", ctgs, {}),
                             ("no contig holds a k-mer", ["ACGT", "N" * 40, "AC"], {})):
            bs, bo = DM.block(cs)
            want = cached(("dedup", name), lambda: DM.dedup(cs, K, **kw))
            d_bs, d_bo = side(device, bs, bo)
            out = kc.dedup_contigs(d_bs, d_bo, **kw)
            early_exits(spy, "kc_ctg_dedup", device, outs=(9, 8, 11, 12), cap=10, totals=(13, 14), stats=15)
            assert out[4] == want["stats"], (name, out[4], want["stats"])
            assert host(out[0]).tobytes() == want["seqs"].tobytes() and (host(out[1], np.uint64) == want["offsets"]).all(), name
            assert host(out[3]).tobytes() == want["records"].tobytes(), name
        assert cached(("dedup", "planted"), None)["stats"]["duplicates"] >= 1 and cached(("dedup", "planted"), None)["stats"]["contained"] >= 1
