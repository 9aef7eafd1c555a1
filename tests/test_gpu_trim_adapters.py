"""kc_trim_adapters on the device against tests/trim_model.py, byte for byte: bases, qualities, offsets and every counter;
both score sets, paired and unpaired; host and device input; the errors; the chain FASTQ -> trim -> merge -> count against
the CPU oracle fed with the model's reads.

The model's side (one Python alignment takes a few milliseconds) was sized to stay in minutes: about one minute per
score set for the 20 000 pairs, under a minute for each of the other tests."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import merge_model as MM
import mhm2_kmer_analysis_v2_amd as pkg
import trim_model as M
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FA_PATH = os.path.join(HERE, "golden", "adapters_no_transposase.fa")
FA = open(FA_PATH, "rb").read()
FA_SEQS = M.read_fasta_seqs(FA_PATH)
STATS = ("reads", "trimmed", "bases_trimmed", "reads_removed", "alignments", "out_bases")


def gpu_trim(kc, b, q, o, paired, device_input=True):
    import torch
    if device_input:
        b, q, o = (torch.from_numpy(np.asarray(x).view(np.int64) if x.dtype == np.uint64 else np.asarray(x)).cuda() for x in (b, q, o))
    ob, oq, oo, st = kc.trim_adapters(b, q, o, paired=paired)
    return ob.cpu().numpy(), oq.cpu().numpy(), oo.cpu().numpy(), st


def check_same(text, k, blastn, b, q, o, modes=(True, False), device_input=True, what=""):
    t0 = time.time()
    ads = M.AdapterSet(text, k, blastn)
    per_read, want = [], {}
    for paired in modes:
        want[paired] = M.trim_reads(ads, b, q, o, paired, per_read)
    t1 = time.time()
    with pkg.KmerCounter(21) as kc:
        kc.load_adapters(text, k, blastn)
        for paired in modes:
            gb, gq, go, gst = gpu_trim(kc, b, q, o, paired, device_input)
            wb, wq, wo, wst = want[paired]
            assert gst == wst, (what, paired, gst, wst)
            assert np.array_equal(go, wo), (what, paired)
            assert np.array_equal(gb, wb) and np.array_equal(gq, wq), (what, paired)
    print("%s: model %.1f s, device %.1f s, %s" % (what, t1 - t0, time.time() - t1, want[modes[0]][3]))
    return want[modes[0]][3]


def test_hand_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "trim_hand_cases.json")))
    assert len(cases) >= 25
    for c in cases:
        b = np.frombuffer("".join(c["reads"]).encode(), dtype=np.uint8)
        q = np.frombuffer(c["quals"].encode(), dtype=np.uint8)
        o = np.cumsum([0] + [len(s) for s in c["reads"]]).astype(np.uint64)
        ads = M.AdapterSet(c["adapters"].encode(), c["k"], c["blastn"])
        wb, wq, wo, wst = M.trim_reads(ads, b, q, o, c["paired"])
        assert np.diff(wo).tolist() == c["expect_lens"] and wst == c["expect_stats"], c["name"]
        with pkg.KmerCounter(21) as kc:
            kc.load_adapters(c["adapters"].encode(), c["k"], c["blastn"])
            for dev in (True, False):
                gb, gq, go, gst = gpu_trim(kc, b, q, o, c["paired"], dev)
                assert gst == wst, (c["name"], gst, wst)
                assert go.tolist() == wo.tolist(), c["name"]
                assert gb.tobytes() == wb.tobytes() and gq.tobytes() == wq.tobytes(), c["name"]


@pytest.mark.parametrize("blastn", [False, True])
def test_random_pairs_20000(blastn):
    b, q, o = M.random_pairs(21 + blastn, 20000, FA_SEQS)
    st = check_same(FA, 21, blastn, b, q, o, what="20000 pairs, blastn=%s" % blastn)
    assert st["trimmed"] > 5000 and st["bases_trimmed"] > 100000 and st["alignments"] > st["trimmed"]


def test_synthetic_big_set_5000_pairs():
    text = M.synthetic_adapters()
    seqs = [l.decode() for l in M.getlines(text) if l[:1] != b">" and len(l) >= 21]
    b, q, o = M.random_pairs(5, 5000, seqs)
    st = check_same(text, 21, False, b, q, o, modes=(True,), what="7500 adapters, 5000 pairs")
    assert st["trimmed"] > 1000


@pytest.mark.parametrize("ln", [250, 300])
def test_longer_reads(ln):
    b, q, o = M.random_pairs(ln, 1500, FA_SEQS, read_len=ln, frag_lo=80, frag_hi=600)
    st = check_same(FA, 21, ln == 300, b, q, o, what="reads of %d" % ln)
    assert st["trimmed"] > 300


def test_reads_of_several_thousand_bases():
    rng = np.random.default_rng(9)
    reads = []
    for i in range(24):
        n = int(rng.integers(1500, 6000))
        s = M._rand_seq(rng, n)
        if i % 3:
            at = int(rng.integers(100, n - 200))
            s = s[:at] + FA_SEQS[int(rng.integers(0, len(FA_SEQS)))] + s[at:]
        if i % 4 == 1:
            s = s + FA_SEQS[2]  # the 119-base entry at the very end
        reads.append(s)
    reads += [M._rand_seq(rng, 32767), M._rand_seq(rng, 20000) + FA_SEQS[0] + M._rand_seq(rng, 3000)]
    b = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    q = rng.integers(35, 74, len(b)).astype(np.uint8)
    o = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
    st = check_same(FA, 21, True, b, q, o, what="long reads")
    assert st["trimmed"] >= 10


def test_long_adapters_take_the_wide_alignment():
    rng = np.random.default_rng(10)
    ads = [M._rand_seq(rng, n) for n in (129, 200, 640, 1024)]
    text = "".join(">l%d\n%s\n" % (i, s) for i, s in enumerate(ads)).encode()
    reads = []
    for i in range(40):
        a = ads[i % 4]
        cut = int(rng.integers(30, len(a) + 1))
        body = M._mutate(rng, a[:cut], int(rng.integers(0, 5)), int(rng.integers(0, 2)))
        reads.append(M._rand_seq(rng, int(rng.integers(0, 200))) + body + (M._rand_seq(rng, 40) if i % 2 else ""))
    b = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    q = rng.integers(35, 74, len(b)).astype(np.uint8)
    o = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
    # 2/3 scores: a score of 254 and more under 1/1/1/1/1 is outside what the rules reproduce (csrc/kc_trim.hpp)
    st = check_same(text, 25, True, b, q, o, modes=(False,), what="adapters of 129..1024 bases")
    assert st["trimmed"] > 20


def test_adapter_free_reads_come_back_unchanged():
    b, q, o = M.random_pairs(3, 20000, FA_SEQS, frag_lo=200, frag_hi=400)
    with pkg.KmerCounter(21) as kc:
        kc.load_adapters(FA_PATH, 21)
        for paired in (True, False):
            gb, gq, go, st = gpu_trim(kc, b, q, o, paired)
            assert st == dict(reads=40000, trimmed=0, bases_trimmed=0, reads_removed=0, alignments=0, out_bases=len(b))
            assert np.array_equal(gb, b) and np.array_equal(gq, q) and np.array_equal(go.astype(np.uint64), o)


def test_host_and_device_input_agree():
    b, q, o = M.random_pairs(4, 3000, FA_SEQS)
    with pkg.KmerCounter(21) as kc:
        kc.load_adapters(FA, 21)
        h = gpu_trim(kc, b, q, o, True, False)
        d = gpu_trim(kc, b, q, o, True, True)
        # host arrays that do not start at offset 0
        h2 = gpu_trim(kc, np.concatenate([np.zeros(7, np.uint8), b]), np.concatenate([np.zeros(7, np.uint8), q]), o + np.uint64(7), True, False)
    for x, y, z in zip(h[:3], d[:3], h2[:3]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert h[3] == d[3] == h2[3] and h[3]["trimmed"] > 500


def test_capacity_state_and_errors():
    import torch
    b, q, o = M.random_pairs(6, 500, FA_SEQS)
    ads = M.AdapterSet(FA, 21)
    wb, wq, wo, want = M.trim_reads(ads, b, q, o, True)
    L = pkg.lib()
    db, dq = torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()
    do = torch.from_numpy(o.view(np.int64)).cuda()
    ob = torch.empty(len(b), dtype=torch.uint8, device="cuda")
    oq = torch.empty(len(b), dtype=torch.uint8, device="cuda")
    oo = torch.empty(1001, dtype=torch.int64, device="cuda")

    def call(kc, n=1000, flags=_lib.KC_TRIM_PAIRED, cap=None, null=False):
        nb, st = C.c_uint64(0), _lib.kc_trim_stats()
        rc = L.kc_trim_adapters(kc._h, db.data_ptr(), dq.data_ptr(), do.data_ptr(), n, 1, flags, None if null else ob.data_ptr(),
                                None if null else oq.data_ptr(), len(b) if cap is None else cap, None if null else oo.data_ptr(),
                                C.byref(nb), C.byref(st))
        return rc, nb.value, {f: int(getattr(st, f)) for f in STATS}

    with pkg.KmerCounter(33) as kc:
        assert call(kc)[0] == _lib.KC_ERR_STATE  # no set loaded: never a silent copy
        with pytest.raises(pkg.KcError) as e:
            kc.load_adapters(FA)  # adapter_k 0 = the context's k = 33
        assert e.value.status == _lib.KC_ERR_UNSUPPORTED_K
        assert call(kc)[0] == _lib.KC_ERR_STATE
        counts = kc.load_adapters(FA, 21)
        assert counts == pkg.adapters_index(FA, 21)
        for cap, null in ((want["out_bases"] - 1, False), (0, False), (0, True)):
            rc, nb, st = call(kc, cap=cap, null=null)
            assert rc == _lib.KC_ERR_CAPACITY and nb == want["out_bases"] and st == want
        rc, nb, st = call(kc, cap=want["out_bases"])
        assert rc == _lib.KC_OK and st == want and np.array_equal(ob[:nb].cpu().numpy(), wb)
        assert call(kc, n=999)[0] == _lib.KC_ERR_INVALID_ARG  # odd and paired
        assert call(kc, n=999, flags=0)[0] == _lib.KC_OK
        assert call(kc, flags=2)[0] == _lib.KC_ERR_INVALID_ARG
        # kc_reset keeps the set
        kc.reset(21)
        rc, nb, st = call(kc)
        assert rc == _lib.KC_OK and st == want
        # loading again replaces it: with one adapter only, fewer reads are trimmed; with the other scores, another result
        kc.load_adapters((">a\n%s\n" % FA_SEQS[0]).encode(), 21)
        rc, nb, st1 = call(kc)
        assert rc == _lib.KC_OK and 0 < st1["trimmed"] < want["trimmed"]
        assert st1 == M.trim_reads(M.AdapterSet((">a\n%s\n" % FA_SEQS[0]).encode(), 21), b, q, o, True)[3]
        # a failed load leaves the loaded set alone
        with pytest.raises(pkg.KcError):
            kc.load_adapters(b">bad\nACGTACGTACGTACGTACGTACGT-\n", 21)
        assert call(kc)[2] == st1
        kc.clear_adapters()
        assert call(kc)[0] == _lib.KC_ERR_STATE
        kc.load_adapters(FA, 21)
        lb = np.full(32768 + 10, ord("A"), np.uint8)
        with pytest.raises(pkg.KcError) as e:
            kc.trim_adapters(lb, lb, np.array([0, 32768, len(lb)], np.uint64))
        assert e.value.status == _lib.KC_ERR_INVALID_ARG
        eb, eq, eo, est = kc.trim_adapters(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        assert eo.cpu().tolist() == [0] and est["reads"] == 0
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        kc.load_adapters(FA, 21)
        gpu_trim(kc, b, q, o, True)
        names = set(kc.kernel_times())
        for n in ("kc_trim_seed_kernel", "kc_trim_align_kernel", "kc_trim_sizes_kernel", "kc_merge_scan_kernel<trim>", "kc_trim_write_kernel"):
            assert n in names, names


def fastq_of(pairs):
    t1, t2 = [], []
    for i, (s1, q1, s2, q2) in enumerate(pairs):
        t1.append(b"@p%d/1\n%s\n+\n%s\n" % (i, s1, q1))
        t2.append(b"@p%d/2\n%s\n+\n%s\n" % (i, s2, q2))
    return b"".join(t1), b"".join(t2)


def chain_pairs(seed, n):
    """pairs from a small genome (so that k-mers repeat), fragments from 40 bases on so that many mates read through
    into an adapter; a few mates are all adapter, or one base of insert, and are cut to 0"""
    rng = np.random.default_rng(seed)
    genome = M._rand_seq(rng, 3000)
    rc = str.maketrans("ACGT", "TGCA")
    pairs = []
    for i in range(n):
        ln = int(rng.integers(100, 151))
        frag = int(rng.integers(40, 320)) if i % 50 else int(rng.integers(0, 12))
        st = int(rng.integers(0, len(genome) - frag))
        g = genome[st:st + frag]
        a1, a2 = FA_SEQS[int(rng.integers(0, len(FA_SEQS)))], FA_SEQS[int(rng.integers(0, len(FA_SEQS)))]
        s1 = (g + a1 + M._rand_seq(rng, 150))[:ln]
        s2 = (g[::-1].translate(rc) + a2 + M._rand_seq(rng, 150))[:ln]
        out = []
        for s in (s1, s2):
            s = list(s)
            for p in rng.integers(0, ln, rng.poisson(0.8)):
                s[p] = "ACGTN"[int(rng.integers(0, 5))]
            out.append("".join(s).encode())
        q1 = bytes(rng.choice([35, 45, 73], ln).astype(np.uint8))
        q2 = bytes(rng.choice([35, 45, 73], ln).astype(np.uint8))
        pairs.append((out[0], q1, out[1], q2))
    return pairs


@pytest.mark.parametrize("k", [21, 33, 77])
def test_chain_matches_oracle(k):
    from oracle import cpu_oracle as O
    pairs = chain_pairs(200 + k, 2500)
    t1, t2 = fastq_of(pairs)
    b, q, o = MM.interleave(pairs)
    blastn = k == 33
    (gk, gc, gl, gr), st, mst = pkg.analyze_kmers_fastq_paired(k, 33, t1, t2, adapters=FA, blastn_scores=blastn, adapter_k=21)
    tb, tq, to, tst = M.trim_reads(M.AdapterSet(FA, 21, blastn), b, q, o, True)
    assert mst["trim"] == tst
    lens = np.diff(to)
    assert (lens == 0).sum() > 10 and tst["trimmed"] > 500
    packed, offs, want = MM.merge_pairs(tb, tq, to.astype(np.uint64), 33, k)
    assert {s: mst[s] for s in want if s in mst and s != "trim"} == {s: want[s] for s in want if s in mst}
    ab, aq, ao = MM.packed_to_ascii(packed, offs)
    orc = O.Oracle(k, nranks=1, nthreads=2)
    orc.add_reads(ab, aq, ao)
    ok, oc, ol, orr = orc.finalize()
    assert gk.shape == ok.shape and (gk == ok).all()
    assert (gc == oc).all() and (gl == ol).all() and (gr == orr).all()
    # the same through analyze_kmers_paired, and adapters=None is today's path
    (pk, pc, pl, pr), _, pmst = pkg.analyze_kmers_paired(k, 33, b, q, o, adapters=FA_PATH, blastn_scores=blastn, adapter_k=21)
    assert (pk == gk).all() and (pc == gc).all() and pmst["trim"] == tst
    (nk, nc, _, _), _, nmst = pkg.analyze_kmers_fastq_paired(k, 33, t1, t2)
    (mk, mc, _, _), _, mmst = pkg.analyze_kmers_paired(k, 33, b, q, o)
    assert "trim" not in nmst and nmst == mmst and nk.shape == mk.shape and (nk == mk).all() and (nc == mc).all()
    upacked, uoffs, uwant = MM.merge_pairs(b, q, o, 33, k)
    assert {s: nmst[s] for s in uwant if s in nmst} == {s: uwant[s] for s in uwant if s in nmst}
    assert nk.shape != gk.shape or not (nk == gk).all()  # trimming changes what is counted


def test_mates_of_length_0_and_1_through_the_merge():
    A = FA_SEQS[0]
    ins = "TTGACCATGCATTGCAAGGCTTACGGATCCATGCAAGTTCAGGCTAACCGTTAGC"
    pairs = [(A[:40], ins), ("G", ins[:30] + A[:30]), (A[:40], A[:40]), (ins, "C"), ("G", "T"), (ins[:5] + A[:34], ins[:40] + A[:30])]
    pairs = [(a.encode(), b"I" * len(a), c.encode(), b"5" * len(c)) for a, c in pairs]
    b, q, o = MM.interleave(pairs)
    tb, tq, to, tst = M.trim_reads(M.AdapterSet(FA, 21), b, q, o, True)
    assert np.diff(to).tolist()[:6] == [0, 55, 1, 30, 0, 0]
    want_p, want_o, want = MM.merge_pairs(tb, tq, to.astype(np.uint64), 33, 21)
    with pkg.KmerCounter(21) as kc:
        kc.load_adapters(FA, 21)
        gb, gq, go, gst = kc.trim_adapters(b, q, o, paired=True)
        assert gst == tst and go.cpu().tolist() == to.tolist()
        packed, offs, mst = kc.merge_pairs(gb, gq, go, min_kmer_len=21)
    assert {s: mst[s] for s in want if s in mst} == {s: want[s] for s in want if s in mst}
    assert np.array_equal(packed.cpu().numpy(), want_p) and np.array_equal(offs.cpu().numpy().view(np.uint64), want_o)


# ---- the seed kernel's own edges -----------------------------------------------------------------------------------------
LONG_AD = [s for s in FA_SEQS if len(s) >= 60][0]


@pytest.mark.parametrize("k", [1, 16, 27, 28, 29, 31, 32])
def test_seed_k(k):
    """k = 1 is the smallest the loader takes (there every fourth base is a seed, so the random reads are kept short for
    the model's sake); 29..32 need the eighth gathered byte, 32 the whole key.  Each k also gets hand-built reads whose
    only indexed k-mer differs from one that is not indexed in a single base."""
    kw = dict(read_len=40, frag_lo=20, frag_hi=80) if k == 1 else {}
    b, q, o = M.random_pairs(300 + k, 2000, FA_SEQS, **kw)
    st = check_same(FA, k, k % 2 == 0, b, q, o, what="adapter_k %d, 2000 pairs" % k)
    assert st["trimmed"] > 200 and st["alignments"] >= st["trimmed"]
    if k == 1:
        # the adapter "A" indexes A and its complement T.  The reads hold C or G at every stride position and anything in
        # between, so nothing is found, until one stride position gets the A (or T) that differs from the C there in
        # that one base; a neighbour of the stride changed the same way stays unseen
        rng = np.random.default_rng(1)
        text = b">one\nA\n"
        ads = M.AdapterSet(text, 1)
        reads = []
        for ln in (1, 4, 5, 9, 40, 225, 229):
            r = list(M._rand_seq(rng, ln))
            r[0::4] = M._rand_seq(rng, len(r[0::4]), "CG")
            reads.append("".join(r))
            for pos in (0, 4, 8, 224, 228, 1, 5, 223):
                if pos < ln:
                    v = list(r)
                    v[pos] = "AT"[pos % 8 == 4]
                    reads.append("".join(v))
        reads += reads[:len(reads) % 2]
        b, q, o = M.reads_to_arrays(reads, seed=1)
        per = M.trim_per_read(ads, b, o)
        nal = {r: x[2] for r, x in zip(reads, per)}
        assert all((nal[r] > 0) == any(c in "AT" for c in r[0::4]) for r in reads) and 10 < sum(1 for v in nal.values() if v) < len(nal) - 10
        check_same(text, 1, False, b, q, o, modes=(False, True), what="adapter_k 1, one base")
        return
    # one adapter of exactly k bases; a read holding it, and reads holding it with one base changed: the last one (which a
    # short mask would not see), the first, and the base behind it (which a long mask would see)
    rng = np.random.default_rng(k)
    while True:
        ad = M._rand_seq(rng, k)
        if ad != M.revcomp(ad.encode()).decode():
            break
    text = (">one\n%s\n" % ad).encode()
    ads = M.AdapterSet(text, k)
    oth = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    reads = []
    for tail in "ACGT":
        fill = tail + M._no_seed_filler(rng, ads, 60)
        reads += [ad + fill, ad[:-1] + oth(ad[-1]) + fill, oth(ad[0]) + ad[1:] + fill, ad[:-1] + oth(oth(ad[-1])) + fill]
    reads += [M._no_seed_filler(rng, ads, 8) + r for r in reads[:8]]
    b, q, o = M.reads_to_arrays(reads, seed=k)
    per = M.trim_per_read(ads, b, o)
    assert [x[2] for x in per[:4]] == [1, 0, 0, 0] and sum(x[2] for x in per) == 6
    check_same(text, k, False, b, q, o, modes=(False, True), what="adapter_k %d, one k-mer" % k)


@pytest.mark.parametrize("k", [21, 29, 32])
def test_seed_positions(k):
    ads = M.AdapterSet(FA, k)
    fam = M.seed_position_reads(ads, LONG_AD, seed=60 + k)
    reads = [r for r, _, _ in fam]
    b, q, o = M.reads_to_arrays(reads + reads[:len(reads) % 2], seed=k)
    st = check_same(FA, k, False, b, q, o, what="seed positions, k %d" % k)
    assert st["alignments"] >= sum(1 for _, _, hit in fam if hit) > 30


@pytest.mark.parametrize("k", [29, 30, 31, 21])
def test_last_read_ends_the_input(k):
    """device arrays sized exactly: the last read's last word has 1-3 bytes (k = 21: a read of 4m + 1 whose last k-mer
    starts on the stride), and its only seed is its last k-mer"""
    ads = M.AdapterSet(FA, k)
    rng = np.random.default_rng(k)
    for m in (0, 1, 13, 56, 57):
        ln = 4 * m + k
        assert ln % 4 in (1, 2, 3)
        last = M._no_seed_filler(rng, ads, 4 * m) + LONG_AD[:k]
        reads = [M._no_seed_filler(rng, ads, 50), last]
        b, q, o = M.reads_to_arrays(reads, seed=m)
        assert M.trim_per_read(ads, b, o)[1][2] == 1
        check_same(FA, k, False, b, q, o, what="last read of %d" % ln)
        # and unpaired with the odd read alone
        b, q, o = M.reads_to_arrays([last], seed=m)
        check_same(FA, k, True, b, q, o, modes=(False,), what="only read of %d" % ln)


def test_any_byte_is_legal():
    b, q, o = M.random_pairs(77, 3000, FA_SEQS)
    rng = np.random.default_rng(78)
    q = rng.integers(0, 256, len(q)).astype(np.uint8)
    odd = np.frombuffer(b"acgtnNRYKMSWBDHVUu0123456789.-*@ \x00\xff", dtype=np.uint8)
    at = rng.integers(0, len(b), len(b) // 25)
    b[at] = rng.choice(odd, len(at))
    lo = rng.integers(0, len(o) - 1, 300)  # whole reads in lower case
    for r in lo:
        b[int(o[r]):int(o[r + 1])] |= 0x20
    st = check_same(FA, 21, False, b, q, o, what="any byte")
    assert st["trimmed"] > 500
    check_same(FA, 31, True, b, q, o, modes=(True,), device_input=False, what="any byte, k 31, 2/3 scores")
