"""kc_merge_pairs on the device against tests/merge_model.py: byte-exact read cache, offsets and counters; host and
device input; KC_ERR_CAPACITY; the whole paired stage against the CPU oracle; qual_offset 64; the seeded families of
merge_model.py aimed at the kernels' own structure (length grid, decisions in later ballot chunks, the long-pair path up
to 32767 bases, device views that start anywhere)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import merge_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ("pairs", "merged", "ambiguous", "dropped", "overlap_len", "merged_len", "out_reads", "out_bases")


def gpu_merge(kc, b, q, o, device_input, min_len=0):
    import torch
    if device_input:
        b, q, o = (torch.from_numpy(np.asarray(x).view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (b, q, o))
    packed, offs, st = kc.merge_pairs(b, q, o, min_kmer_len=min_len)
    return packed.cpu().numpy(), offs.cpu().numpy().view(np.uint64), st


def check_same(b, q, o, k=21, min_len=21, device_input=True, qoff=33):
    want_p, want_o, want_st = M.merge_pairs(b, q, o, qoff, min_len)
    with pkg.KmerCounter(k, qual_offset=qoff) as kc:
        got_p, got_o, got_st = gpu_merge(kc, b, q, o, device_input, min_len)
    assert {s: got_st[s] for s in STATS} == {s: want_st[s] for s in STATS}
    assert np.array_equal(got_o, want_o)
    if not np.array_equal(got_p, want_p):
        bad = int(np.nonzero(got_p != want_p)[0][0])
        pytest.fail("packed bytes differ first at %d: %d != %d" % (bad, got_p[bad], want_p[bad]))
    return want_st


def test_hand_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "merge_hand_cases.json")))["cases"]
    for c in cases:
        b, q, o = M.interleave([c["pair"]])
        with pkg.KmerCounter(21) as kc:
            p, offs, st = gpu_merge(kc, b, q, o, True, c["min_kmer_len"])
        assert p.tolist() == c["packed"], c["name"]
        assert offs.tolist() == c["offsets"], c["name"]
        assert {s: st[s] for s in c["stats"]} == c["stats"], c["name"]
    # all of them in one batch
    b, q, o = M.interleave([c["pair"] for c in cases if c["min_kmer_len"] == 21])
    check_same(b, q, o)


def test_random_pairs_20000():
    rng = np.random.default_rng(11)
    b, q, o = M.interleave(M.random_pairs(rng, 20000, 1, 300))
    st = check_same(b, q, o)
    assert st["merged"] > 5000 and st["ambiguous"] > 50 and st["dropped"] > 100


@pytest.mark.parametrize("ln", [250, 300])
def test_full_length_batches(ln):
    rng = np.random.default_rng(ln)
    b, q, o = M.interleave(M.random_pairs(rng, 3000, ln, ln))
    check_same(b, q, o)


def test_long_pairs_take_the_generic_path():
    rng = np.random.default_rng(5)
    pairs = M.random_pairs(rng, 40, 400, 5000) + M.random_pairs(rng, 200, 100, 200)
    rng.shuffle(pairs)
    b, q, o = M.interleave(pairs)
    st = check_same(b, q, o)
    assert st["merged"] > 10


def test_host_and_device_input_agree():
    rng = np.random.default_rng(12)
    b, q, o = M.interleave(M.random_pairs(rng, 3000, 1, 300))
    with pkg.KmerCounter(21) as kc:
        hp, ho, hs = gpu_merge(kc, b, q, o, False)
        dp, do, ds = gpu_merge(kc, b, q, o, True)
    assert np.array_equal(hp, dp) and np.array_equal(ho, do) and hs == ds


def test_capacity_and_errors():
    import torch
    rng = np.random.default_rng(13)
    b, q, o = M.interleave(M.random_pairs(rng, 500, 1, 300))
    _, want_o, want = M.merge_pairs(b, q, o)
    L = pkg.lib()
    with pkg.KmerCounter(21) as kc:
        db, dq = torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()
        do = torch.from_numpy(o.view(np.int64)).cuda()
        out = torch.empty(len(b), dtype=torch.uint8, device="cuda")
        oo = torch.empty(1001, dtype=torch.int64, device="cuda")
        for cap_b, cap_r in ((want["out_bases"] - 1, 1000), (len(b), want["out_reads"] - 1), (0, 0)):
            n, nb, st = C.c_uint64(0), C.c_uint64(0), _lib.kc_merge_stats()
            rc = L.kc_merge_pairs(kc._h, db.data_ptr(), dq.data_ptr(), do.data_ptr(), 500, 1, 0, out.data_ptr() if cap_b else None, cap_b,
                                  oo.data_ptr() if cap_r else None, cap_r, C.byref(n), C.byref(nb), C.byref(st))
            assert rc == _lib.KC_ERR_CAPACITY
            assert (n.value, nb.value) == (want["out_reads"], want["out_bases"])
            assert st.merged == want["merged"] and st.out_bases == want["out_bases"]
        # a byte outside the table, a quality outside [33, 113], a mate longer than 32767
        for bad in ("base", "qual_low", "qual_high"):
            b2, q2 = b.copy(), q.copy()
            if bad == "base":
                b2[int(o[7])] = ord("X")
            elif bad == "qual_low":
                q2[int(o[7])] = 32
            else:
                q2[int(o[7])] = 33 + 81
            with pytest.raises(pkg.KcError) as e:
                kc.merge_pairs(b2, q2, o)
            assert e.value.status == (_lib.KC_ERR_BAD_BASE if bad == "base" else _lib.KC_ERR_INVALID_ARG)
        lb = np.full(32768 + 10, ord("A"), np.uint8)
        with pytest.raises(pkg.KcError) as e:
            kc.merge_pairs(lb, np.full(len(lb), 73, np.uint8), np.array([0, 32768, len(lb)], np.uint64))
        assert e.value.status == _lib.KC_ERR_INVALID_ARG


@pytest.mark.parametrize("k", [21, 33, 77])
def test_paired_stage_matches_oracle(k):
    from oracle import cpu_oracle as O
    rng = np.random.default_rng(100 + k)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 3000)
    pairs = []
    for _ in range(3000):  # fragments of a small genome, so that k-mers repeat
        ln = int(rng.integers(60, 151))
        frag = int(rng.integers(ln, 2 * ln + 10))
        st = int(rng.integers(0, len(genome) - frag))
        g = genome[st:st + frag]
        s1, s2 = g[:ln].copy(), M.COMP[g[frag - ln:][::-1]].copy()
        q1 = rng.choice([35, 45, 73], ln).astype(np.uint8)
        q2 = rng.choice([35, 45, 73], ln).astype(np.uint8)
        for s in (s1, s2):
            for p in rng.integers(0, ln, rng.poisson(1.0)):
                s[p] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8))
        pairs.append((s1.tobytes(), q1.tobytes(), s2.tobytes(), q2.tobytes()))
    b, q, o = M.interleave(pairs)
    (gk, gc, gl, gr), st, mst = pkg.analyze_kmers_paired(k, 33, b, q, o)
    packed, offs, want = M.merge_pairs(b, q, o, 33, k)
    assert {s: mst[s] for s in STATS} == {s: want[s] for s in STATS}
    ab, aq, ao = M.packed_to_ascii(packed, offs)
    orc = O.Oracle(k, nranks=1, nthreads=2)
    orc.add_reads(ab, aq, ao)
    ok, oc, ol, orr = orc.finalize()
    assert gk.shape == ok.shape and (gk == ok).all()
    assert (gc == oc).all() and (gl == ol).all() and (gr == orr).all()
    assert want["merged"] > 500


def test_two_million_pairs():
    import torch
    n = 2_000_000
    with pkg.KmerCounter(21) as kc:
        p = pkg.synth_params(read_len=150)
        fb = torch.empty(n * 150, dtype=torch.uint8, device="cuda")
        fq = torch.empty(n * 150, dtype=torch.uint8, device="cuda")
        fo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        kc.synth_reads_device(fb, fq, fo, n, params=p)
        # mate 1: the first 100 bases of a read; mate 2: reverse complement of its last 100
        f = fb.view(n, 150)
        fq2 = fq.view(n, 150)
        comp = torch.zeros(256, dtype=torch.uint8, device="cuda")
        for a, c in zip(b"ACGTN", b"TGCAN"):
            comp[a] = c
        m1, m2 = f[:, :100], comp[f[:, 50:].flip(1).long()]
        bases = torch.stack([m1, m2], 1).reshape(-1)
        quals = torch.stack([fq2[:, :100], fq2[:, 50:].flip(1)], 1).reshape(-1)
        offs = torch.arange(0, 2 * n + 1, device="cuda", dtype=torch.int64) * 100
        packed, oo, st = kc.merge_pairs(bases, quals, offs)
    assert st["pairs"] == n and st["merged"] > n // 2
    assert st["out_reads"] == 2 * n - st["merged"] - 2 * st["dropped"]
    assert st["out_bases"] == len(packed) == int(oo[-1].item())
    assert int(oo[0].item()) == 0 and len(oo) == st["out_reads"] + 1
    lens = oo[1:] - oo[:-1]
    assert int(lens.min().item()) >= 100  # offsets never decrease; a merged read has 100..200 bases, any other 100
    assert int(lens.max().item()) <= 200 and int((lens != 100).sum().item()) <= st["merged"]
    assert int(lens.sum().item()) == 100 * (st["out_reads"] - st["merged"]) + st["merged_len"]


# ---- qual_offset 64 ----------------------------------------------------------------------------------------------------
def shifted(pair, by=31):
    return (pair[0], bytes(c + by for c in pair[1].encode()), pair[2], bytes(c + by for c in pair[3].encode()))


def test_qual_offset_64_hand_cases():
    cases = [c for c in json.load(open(os.path.join(HERE, "golden", "merge_hand_cases.json")))["cases"] if c["qual_offset"] == 33]
    assert len(cases) >= 18
    for c in cases:
        b, q, o = M.interleave([shifted(c["pair"])])
        with pkg.KmerCounter(21, qual_offset=64) as kc:
            p, offs, st = gpu_merge(kc, b, q, o, True, c["min_kmer_len"])
        assert p.tolist() == c["packed"], c["name"]
        assert offs.tolist() == c["offsets"], c["name"]
        assert {s: st[s] for s in c["stats"]} == c["stats"], c["name"]
    b, q, o = M.interleave([shifted(c["pair"]) for c in cases if c["min_kmer_len"] == 21])
    check_same(b, q, o, qoff=64)
    check_same(b, q, o, qoff=64, device_input=False)


def test_qual_offset_64_random_pairs_5000():
    rng = np.random.default_rng(64)
    b, q, o = M.interleave(M.random_pairs(rng, 5000, 1, 300, qoff=64))
    st = check_same(b, q, o, qoff=64)
    assert st["merged"] > 1200 and st["ambiguous"] > 10 and st["dropped"] > 25
    assert st["out_reads"] - st["merged"] > 2000  # unmerged mates: mate 2 goes out from its own qualities


def test_qual_offset_64_paired_stage_matches_oracle():
    from oracle import cpu_oracle as O
    k = 21
    rng = np.random.default_rng(164)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 3000)
    pairs = []
    for _ in range(3000):
        ln = int(rng.integers(60, 151))
        frag = int(rng.integers(ln, 2 * ln + 10))
        st = int(rng.integers(0, len(genome) - frag))
        g = genome[st:st + frag]
        s1, s2 = g[:ln].copy(), M.COMP[g[frag - ln:][::-1]].copy()
        q1 = rng.choice([66, 76, 104], ln).astype(np.uint8)
        q2 = rng.choice([66, 76, 104], ln).astype(np.uint8)
        for s in (s1, s2):
            for p in rng.integers(0, ln, rng.poisson(1.0)):
                s[p] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8))
        pairs.append((s1.tobytes(), q1.tobytes(), s2.tobytes(), q2.tobytes()))
    b, q, o = M.interleave(pairs)
    (gk, gc, gl, gr), st, mst = pkg.analyze_kmers_paired(k, 64, b, q, o)
    packed, offs, want = M.merge_pairs(b, q, o, 64, k)
    assert {s: mst[s] for s in STATS} == {s: want[s] for s in STATS}
    ab, aq, ao = M.packed_to_ascii(packed, offs, 64)
    orc = O.Oracle(k, 64, nranks=1, nthreads=2)
    orc.add_reads(ab, aq, ao)
    ok, oc, ol, orr = orc.finalize()
    assert gk.shape == ok.shape and (gk == ok).all()
    assert (gc == oc).all() and (gl == ol).all() and (gr == orr).all()
    assert want["merged"] > 500


def test_qual_offset_64_errors():
    rng = np.random.default_rng(13)
    b, q, o = M.interleave(M.random_pairs(rng, 500, 1, 300, qoff=64))
    with pkg.KmerCounter(21, qual_offset=64) as kc:
        kc.merge_pairs(b, q, o)
        for bad in (63, 64 + 81):
            q2 = q.copy()
            q2[int(o[7])] = bad
            with pytest.raises(pkg.KcError) as e:
                kc.merge_pairs(b, q2, o)
            assert e.value.status == _lib.KC_ERR_INVALID_ARG
        q2 = q.copy()
        q2[int(o[7])], q2[int(o[9])] = 64, 64 + 80  # the ends of the range are legal
        kc.merge_pairs(b, q2, o)
        b33, q33, o33 = M.interleave([("ACGT" * 10, "5" * 40, "TTGCA" * 8, "I" * 40)])  # valid at 33: qualities 20 and 40
        with pytest.raises(pkg.KcError) as e:
            kc.merge_pairs(b33, q33, o33)
        assert e.value.status == _lib.KC_ERR_INVALID_ARG
    with pkg.KmerCounter(21) as kc:
        assert kc.merge_pairs(b33, q33, o33)[2]["pairs"] == 1


# ---- the kernels' own edges ----------------------------------------------------------------------------------------------
def test_length_grid():
    pairs = M.length_grid_pairs()
    b, q, o = M.interleave(pairs)
    st = check_same(b, q, o)
    assert st["merged"] > 3000 and st["dropped"] >= 9
    check_same(b, q, o, device_input=False)
    b, q, o = M.interleave(M.length_grid_pairs(seed=32, qoff=64)[::3])
    check_same(b, q, o, qoff=64)


def test_cross_chunk_decisions():
    pairs = M.cross_chunk_pairs()
    b, q, o = M.interleave(pairs)
    st = check_same(b, q, o)
    assert st["merged"] * 5 >= len(pairs) and st["ambiguous"] > 800
    # with Ns sprinkled in, the same decisions are replayed by the write pass
    rng = np.random.default_rng(42)
    noisy = []
    for s1, q1, s2, q2 in M.cross_chunk_pairs(seed=43, n=800):
        s1, s2 = bytearray(s1), bytearray(s2)
        s1[int(rng.integers(0, len(s1)))] = M.N
        if rng.random() < 0.5:
            s2[int(rng.integers(0, len(s2)))] = M.N
        noisy.append((bytes(s1), q1, bytes(s2), q2))
    b, q, o = M.interleave(noisy)
    st = check_same(b, q, o)
    assert st["merged"] > 50 and st["ambiguous"] > 300


def test_long_path_edges():
    rng = np.random.default_rng(52)
    pairs = M.long_path_pairs() + M.random_pairs(rng, 600, 1, 300)
    rng.shuffle(pairs)  # long and short pairs share tiles
    b, q, o = M.interleave(pairs)
    st = check_same(b, q, o)
    assert st["merged"] > 200 and st["merged_len"] > 32767 + 3 * 20000
    check_same(b, q, o, device_input=False)
    # long pairs that min_kmer_len drops
    short = [p for p in pairs if max(len(p[0]), len(p[2])) <= 520]
    b, q, o = M.interleave(short)
    st = check_same(b, q, o, min_len=600)
    assert st["dropped"] == len(short) and st["out_reads"] == 0
    st = check_same(b, q, o, min_len=516)
    assert 0 < st["dropped"] < len(short)


def test_device_views_that_start_anywhere():
    import torch
    rng = np.random.default_rng(53)
    pairs = M.random_pairs(rng, 700, 1, 300) + M.long_path_pairs()[3:12]
    b, q, o = M.interleave(pairs)
    want_p, want_o, want_st = M.merge_pairs(b, q, o)
    with pkg.KmerCounter(21) as kc:
        for res in range(4):
            for shift in (1, 2, 3, 4, 1001):
                big_b = torch.full((len(b) + 2048,), ord("X"), dtype=torch.uint8, device="cuda")  # X: no legal base
                big_q = torch.zeros(len(b) + 2048, dtype=torch.uint8, device="cuda")               # 0: no legal quality
                vb, vq = big_b[res:], big_q[res:]
                vb[shift:shift + len(b)] = torch.from_numpy(b).cuda()
                vq[shift:shift + len(b)] = torch.from_numpy(q).cuda()
                assert vb.data_ptr() % 4 == (big_b.data_ptr() + res) % 4
                vo = torch.from_numpy((o + np.uint64(shift)).view(np.int64)).cuda()
                packed, offs, st = kc.merge_pairs(vb, vq, vo)
                assert {s: st[s] for s in STATS} == {s: want_st[s] for s in STATS}, (res, shift)
                assert np.array_equal(offs.cpu().numpy().view(np.uint64), want_o), (res, shift)
                assert np.array_equal(packed.cpu().numpy(), want_p), (res, shift)
