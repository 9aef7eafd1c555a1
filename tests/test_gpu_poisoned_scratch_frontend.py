"""The read front end (FASTQ parse, pair merge, adapter trim, FASTQ and FASTA text) and the shard flows on memory that is
not zero when the library gets it: KC_DEBUG_FILL fills every fresh allocation of the library ("Poisoned
scratch"), 0xA5 and 0x5A a case, and every result still equals its model exactly -- the host parser of the same library for
the FASTQ parse (no reference independent of the library by itself: the host parser is pinned, without a GPU, to PackedRead's
byte rule written out in Python, to the reference's line and error rules and to hand cases by tests/test_fastq.py and
tests/test_fastq_pairs.py), tests/merge_model.py, tests/trim_model.py, tests/fastq_out_model.py, tests/fasta_in_model.py, and the CPU
oracle for the shard flows.  The expectations are computed once a case and cached; only the device calls are repeated per
fill.  Contexts are made after the variable is set, and every test checks that kc_debug_filled_bytes() rose.

Shapes: a tile of the merge is 64 pairs (65: a tile and a pair; 64 dropped pairs in front: a tile that writes nothing), of
the trim 256 reads (257: a tile and a read), of the line index 64 KiB of text (a text of 70 000 bytes ends mid-tile).  Every
family is called on one context in a larger-then-smaller order too, so that the kept blocks (mg, tr, fq_*, the staging) hold
another call's bytes.  Wall time on the MI355X: 4 s for the module's 30 tests."""
import numpy as np
import pytest

import fasta_in_cases as FAC
import fasta_in_model as FAM
import fastq_out_cases as FQC
import fastq_out_model as FQM
import merge_model as MM
import mhm2_kmer_analysis_v2_amd as pkg
import trim_model as TM
from helpers import random_reads
from mhm2_kmer_analysis_v2_amd import _lib
from test_gpu_fasta_in import exact as fasta_exact
from test_gpu_fasta_in import model as fasta_model
from test_gpu_fastq import HAND, gen_text, make_records, render, same_packed, same_pairs
from test_gpu_fastq_out import source as fq_source
from test_gpu_merge_pairs import STATS as MG_STATS
from test_gpu_merge_pairs import gpu_merge
from test_gpu_parity import PATHS, arrays, assert_same, oracle_run
from test_gpu_shard_flow import run_shards, union
from test_gpu_trim_adapters import FA, FA_SEQS, gpu_trim
from test_gpu_wire6 import run_flow

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)


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


# ---- FASTQ parse -----------------------------------------------------------------------------------------------------------
def fastq_texts():
    """sound texts of 300 records; one of 70 000 bytes that ends inside its second tile of the line index, with empty records
    (no bases) among the others and no newline at its end; and the hand cases: empty, truncated and malformed texts"""
    def make():
        rng = np.random.default_rng(4100)
        sound = render(rng, make_records(rng, 300), style=0)
        recs = make_records(rng, 2400, max_len=20)
        for i in range(0, len(recs), 7):
            recs[i][1] = recs[i][3] = b""
        long = render(rng, recs, style=0)[:70000]
        long = long[:long.rindex(b"\n@")]
        assert 65536 < len(long) < 2 * 65536 and not long.endswith(b"\n")
        fuzz = [gen_text(rng) for _ in range(40)]
        return sound, long, fuzz
    return cached("fastq", make)


def test_fastq_parse(fill):
    sound, long, fuzz = fastq_texts()
    with pkg.KmerCounter(21) as kc:
        for dev in (False, True):
            for t in (long, sound, b"", long[:3000]) + tuple(HAND) + tuple(fuzz):  # (smaller texts behind larger ones)
                same_packed(kc, t, 33, dev)
            for t1, t2 in ((long, None), (sound, sound), (sound, None), (b"", None), (HAND[4], b""), (long[:5000], long[:3000])):
                same_pairs(kc, t1, t2, dev)
            # a size query and a capacity one short
            want = same_packed(kc, sound, 33, dev, arrays=False)
            same_packed(kc, sound, 33, dev, cap=want[2] - 1)
            same_packed(kc, sound, 33, dev, rcap=want[1] - 1)


# ---- pair merge --------------------------------------------------------------------------------------------------------------
def merge_cases():
    def make():
        rng = np.random.default_rng(4200)
        ordinary = MM.random_pairs(rng, 65, 1, 300)
        short = [(s1[:int(rng.integers(0, 15))], q1[:0], s2[:int(rng.integers(0, 15))], q2[:0]) for s1, q1, s2, q2 in MM.random_pairs(rng, 64, 20, 40)]
        short = [(s1, np.full(len(s1), 40, np.uint8).tobytes(), s2, np.full(len(s2), 40, np.uint8).tobytes()) for s1, _, s2, _ in short]
        long = MM.random_pairs(rng, 3, 400, 900)  # the long-pair list
        out = {}
        for name, pairs in (("65 pairs", ordinary), ("a tile of dropped pairs, then 65", short + ordinary), ("long pairs among them", ordinary[:40] + long + ordinary[40:]),
                            ("one pair", ordinary[:1])):
            b, q, o = MM.interleave(pairs)
            out[name] = ((b, q, o), MM.merge_pairs(b, q, o, 33, 21))
        assert out["a tile of dropped pairs, then 65"][1][2]["dropped"] >= 64
        return out
    return cached("merge", make)


def test_merge_pairs(fill):
    with pkg.KmerCounter(21) as kc:
        for dev in (True, False):
            for name in ("long pairs among them", "a tile of dropped pairs, then 65", "65 pairs", "one pair"):
                (b, q, o), (want_p, want_o, want_st) = merge_cases()[name]
                got_p, got_o, got_st = gpu_merge(kc, b, q, o, dev, 21)
                assert {s: got_st[s] for s in MG_STATS} == {s: want_st[s] for s in MG_STATS}, name
                assert np.array_equal(got_o, want_o) and np.array_equal(got_p, want_p), name
        e = np.zeros(0, dtype=np.uint8)
        p, offs, st = kc.merge_pairs(e, e, np.zeros(1, dtype=np.uint64))  # no pairs
        assert len(p) == 0 and offs.cpu().tolist() == [0] and st["pairs"] == 0 and st["out_reads"] == 0


# ---- adapter trim ------------------------------------------------------------------------------------------------------------
def trim_cases():
    def make():
        ads = TM.AdapterSet(FA, 21, False)
        b, q, o = TM.random_pairs(4300, 129, FA_SEQS)
        cut = int(o[257])
        free = TM.random_pairs(4301, 40, FA_SEQS, frag_lo=200, frag_hi=400)  # fragments longer than the reads: no adapter
        out = {"258 reads, paired": ((b, q, o), True), "257 reads": ((b[:cut], q[:cut], o[:258]), False), "80 reads without a hit": (free, True)}
        want = {name: TM.trim_reads(ads, *a, paired) for name, (a, paired) in out.items()}
        assert want["258 reads, paired"][3]["trimmed"] >= 30 and want["80 reads without a hit"][3]["alignments"] == 0
        return out, want
    return cached("trim", make)


def test_trim_adapters(fill):
    cases, want = trim_cases()
    with pkg.KmerCounter(21) as kc:
        kc.load_adapters(FA, 21, False)
        for dev in (True, False):
            for name in ("258 reads, paired", "80 reads without a hit", "257 reads"):
                (b, q, o), paired = cases[name]
                gb, gq, go, gst = gpu_trim(kc, b, q, o, paired, dev)
                wb, wq, wo, wst = want[name]
                assert gst == wst, (name, gst, wst)
                assert np.array_equal(go, wo) and np.array_equal(gb, wb) and np.array_equal(gq, wq), name


# ---- FASTQ text --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", (False, True), ids=("ascii", "packed"))
def test_fastq_text(fill, packed):
    def make():
        out = {}
        for name, reads in (("edge", FQC.edge_reads()), ("small", FQC.small_reads())):
            b, q = fq_source(reads, packed)
            out[name] = (b, q, reads[2], FQM.fastq(b, q, reads[2], prefix="r", paired=True))
        return out
    cases = cached(("fastq text", packed), make)
    with pkg.KmerCounter(21) as kc:
        for dev in (False, True):
            for name in ("edge", "small"):
                b, q, o, want = cases[name]
                for shift, src_shift in ((0, 0), (7, 15)):
                    rc, got, w, total = FQC.text_call(kc, b, q, o, prefix="r", flags=FQM.PAIRED, capacity=len(want), dev=dev, shift=shift, src_shift=src_shift)
                    assert rc == 0 and (w, total) == (len(want), len(want)) and got == want, (name, shift)
                # a window in the middle, a size query, a capacity one short of the whole
                rc, got, w, total = FQC.text_call(kc, b, q, o, flags=FQM.PAIRED, first_byte=5, capacity=len(want) - 9, dev=dev, shift=3)
                assert rc == 0 and total == len(want) and got == FQM.window(want, 5, len(want) - 9), name
                rc, got, w, total = FQC.text_call(kc, b, q, o, flags=FQM.PAIRED, capacity=1 << 20, dev=dev, query=True)
                assert (rc, got, w, total) == (0, b"", 0, len(want)), name
                rc, got, w, total = FQC.text_call(kc, b, q, o, flags=FQM.PAIRED, capacity=len(want) - 1, dev=dev)
                assert rc == 0 and total == len(want) and got == want[:-1], name
            db, dq, do = FQC.on(dev, *cases["edge"][:3])
            assert kc.fastq_text(db, dq, do, paired=True, check=True) == cases["edge"][3]
        e = np.zeros(0, dtype=np.uint8)
        assert kc.fastq_text(e, None if packed else e, np.zeros(1, dtype=np.uint64)) == b""  # no reads


# ---- FASTA text to block -----------------------------------------------------------------------------------------------------
def test_fasta_to_block(fill):
    with pkg.KmerCounter(21) as kc:
        for dev in (False, True):
            for last in ("header", "bases"):
                for text_shift, shift in ((0, 0), (3, 6)):
                    fasta_exact(kc, FAC.edge_text(last), 0, 9, dev, text_shift=text_shift, shift=shift)
            fasta_exact(kc, FAC.small_text()[:300], 0, 3, dev, shift=1)  # (a smaller text behind a larger one)
            fasta_exact(kc, FAC.small_text()[:300], FAM.PARTIAL, 3, dev, shift=2)
            for text in (b"", b"\n", b"\n\r\n \t\n\n", b" ", b">", b">x", b">x\n", b">x\r\n\n", b">x 5\nA", b">\nA\n"):  # the smallest texts
                for flags in (0, FAM.PARTIAL):
                    got = fasta_exact(kc, text, flags, 3, dev, shift=1)
                    assert got["status"] == 0 and got["n_ctgs"] == (0 if flags else text.count(b">"))
            # a size query, and arrays one short: the totals and nothing else
            want = fasta_model(FAC.edge_text(), 0, 0)
            n, c = len(want["seqs"]), len(want["offsets"]) - 1
            FAC.same(FAC.call(kc, FAC.edge_text(), 0, 0, dev, query=True), want)
            for short in (dict(seqs_capacity=n - 1, ctgs_capacity=c), dict(seqs_capacity=n, ctgs_capacity=c - 1)):
                got = FAC.call(kc, FAC.edge_text(), 0, 0, dev, shift=5, **short)
                assert got["status"] == _lib.KC_ERR_CAPACITY and (got["n_ctgs"], got["nbytes"]) == (c, n)


# ---- shard flows: two shards on the one GPU ----------------------------------------------------------------------------------
def shard_case(k, lonely):
    """about 600 reads; lonely: the first half gives no k-mer (shorter than k), so that the second shard receives nothing"""
    def make():
        rng = np.random.default_rng(4400 + k)
        reads, quals = random_reads(rng, 600, min_len=30, max_len=150, genome_len=900, err=0.01)
        if lonely:
            half = (len(reads) + 1) // 2
            reads = [r[:k - 1] for r in reads[:half]] + reads[half:]
            quals = [x[:k - 1] for x in quals[:half]] + quals[half:]
        b, q, offs = arrays(reads, quals)
        return reads, quals, oracle_run(b, q, offs, k)
    return cached(("shard", k, lonely), make)


@pytest.mark.parametrize("lonely", (False, True), ids=("ordinary", "a shard that receives nothing"))
@pytest.mark.parametrize("k,path", [(21, "compact-short"), (33, "bucketed-small")])
def test_single_pass_shard_flow(fill, k, path, lonely):
    reads, quals, (want, _, wst) = shard_case(k, lonely)
    shards, shipped, total = run_shards(reads, quals, k, 2, PATHS[path])
    try:
        parts = [s.sorted_results() for s in shards]
        assert_same(union(parts), want)
        st = [s.stats() for s in shards]
        assert sum(x["kmers_inserted"] for x in st) == wst["kmers_inserted"] == total
        assert sum(x["num_unique"] for x in st) == wst["unique"] and sum(x["num_purged"] for x in st) == wst["purged"]
    finally:
        for s in shards:
            s.close()


@pytest.mark.parametrize("lonely", (False, True), ids=("ordinary", "a block without k-mers"))
@pytest.mark.parametrize("wire_units", (False, True), ids=("k-mer records", "wire units"))
def test_records_flow(fill, wire_units, lonely):
    k = 21
    reads, quals, (want, _, wst) = shard_case(k, lonely)
    shards, _, _ = run_flow(reads, quals, k, 2, PATHS["compact-short"], blocks=2, wire_units=wire_units)
    try:
        parts = [s.sorted_results() for s in shards]
        assert_same(union(parts), want)
        assert sum(s.stats()["kmers_inserted"] for s in shards) == wst["kmers_inserted"]
        for r, (s, p) in enumerate(zip(shards, parts)):
            for i in range(0, len(p[1]), 29):
                assert s.partition_owner(p[0][i]) == r
    finally:
        for s in shards:
            s.close()


def test_seq_block_senders_and_record_pieces(fill):
    """the senders that read the '_'-joined case-masked block (kc_shard_extract_seq_block, kc_extract_partition_seq_block), and
    the receiver that takes a destination's pieces where they lie (kc_insert_record_pieces)"""
    import torch
    k, R = 21, 2
    reads, quals, (want, _, wst) = shard_case(k, False)
    masked = cached("masked", lambda: ["".join(c.lower() if ord(x) < 33 + 20 else c for c, x in zip(r, ql)) for r, ql in zip(reads, quals)])
    # wire units, the pieces of a destination in one call
    shards, (uw, ur, Q), _ = run_flow(reads, quals, k, R, PATHS["compact-short"], blocks=3, together="strided")
    try:
        assert (uw, ur) == (3, 4) and Q > 1
        assert_same(union([s.sorted_results() for s in shards]), want)
        assert sum(s.stats()["kmers_inserted"] for s in shards) == wst["kmers_inserted"]
    finally:
        for s in shards:
            s.close()
    # the single-pass flow from seq blocks, one of them empty
    shards = [pkg.KmerCounter(k, rank_me=r, rank_n=R, tuning=PATHS["compact"]) for r in range(R)]
    try:
        seg_words = sum(max(0, len(r) - k - 1) for r in reads) * shards[0].rec_nl + 2048
        segs = torch.zeros(R * seg_words, dtype=torch.int64, device="cuda")
        for r in range(R):
            for part in (masked[r::R][0::2], [], masked[r::R][1::2]):
                words = shards[r].shard_extract_seq_block("_".join(part).encode(), segs, seg_words)
                for d in range(R):
                    w = int(words[d])
                    if d == r or not w:
                        continue
                    dst = shards[d].shard_reserve(w)
                    dst.copy_(segs[d * seg_words:d * seg_words + w])
                    torch.cuda.synchronize()
                    shards[d].shard_commit(dst, w)
        assert_same(union([s.sorted_results() for s in shards]), want)
        assert sum(s.stats()["kmers_inserted"] for s in shards) == wst["kmers_inserted"]
    finally:
        for s in shards:
            s.close()
    # the records flow from a seq block, in wire units
    shards = [pkg.KmerCounter(k, rank_me=r, rank_n=R, tuning=PATHS["compact-short"], wire_units=True) for r in range(R)]
    try:
        block = np.frombuffer(("_".join(masked) + "_").encode(), dtype=np.uint8)
        uw, ur, Q = shards[0].wire_unit()
        seg = len(block) // ur + 8 * 1024
        recs = torch.zeros(R * Q * seg * uw, dtype=torch.int64, device="cuda")
        counts = np.zeros(R * Q, dtype=np.uint64)
        _lib.check(pkg.lib().kc_extract_partition_seq_block(shards[0]._h, block.ctypes.data, len(block), 0, recs.data_ptr(), seg, counts.ctypes.data),
                   "kc_extract_partition_seq_block")
        for j in range(R * Q):
            if int(counts[j]):
                shards[j // Q].insert_records(recs[j * seg * uw:], int(counts[j]))
        assert_same(union([s.sorted_results() for s in shards]), want)
    finally:
        for s in shards:
            s.close()
