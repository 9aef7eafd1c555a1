"""Level 1's two bookkeeping phases against the oracle, bit-exact: the staging of a tile (csrc/kc_encode.hpp: codes, ok bits,
separators and the bad-byte flag, four bytes per instruction) and the copy-out of a round (csrc/kc_bucketed.hpp,
split_stage_pairs / split_copy_out_pairs: a fast path for the trips whose runs all lie in one chunk, the general one for the
rest).  Every input has at most 4000 reads; an input's oracle result is computed once and shared."""
import functools

import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
from oracle import cpu_oracle as O
from helpers import random_reads

pytestmark = pytest.mark.gpu

CUT = 33 + 20                    # qual_offset + the quality cutoff
SIX = dict(p1=1024, p2=1024)     # the benchmark's fan-outs: six-byte level-1 records at k = 21 (kc_l1_reads16_kernel)
BAD_BASE = -7


def assert_same(got, want):
    for g, w, name in zip(got, want, ("keys", "counts", "left", "right")):
        assert g.shape == w.shape, "%s: %s vs %s" % (name, g.shape, w.shape)
        assert (g == w).all(), name


def oracle(reads, quals, k):
    b, q, offs = O.reads_to_arrays(reads, quals)
    o = O.Oracle(k, nranks=3, nthreads=4)
    o.add_reads(b, q, offs)
    want = o.finalize()
    assert o.stats()["dropped"] == 0
    o.close()
    return want


# ---- staging ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def staging_reads(nreads):
    """reads of 23-300 bases in both cases with Ns; the qualities cut - 1, cut, cut + 1, 33 and 126 on the last byte of
    every four-byte word and the first of the next (so, at any alignment of the array, on both sides of every word and
    group boundary), high and low ones elsewhere"""
    rng = np.random.default_rng(606)
    reads, _ = random_reads(rng, nreads, min_len=23, max_len=300, genome_len=5000, err=0.01, n_rate=0.01)
    reads = ["".join(c.lower() if rng.random() < 0.3 else c for c in r) for r in reads]
    vals = [CUT - 1, CUT, CUT + 1, 33, 126]
    quals, i = [], 0
    for r in reads:
        q = []
        for _ in r:
            if i % 4 in (3, 0):
                q.append(vals[(i // 4 + i) % 5])
            else:
                q.append(73 if rng.random() < 0.9 else 35)
            i += 1
        quals.append("".join(chr(x) for x in q))
    return tuple(reads), tuple(quals)


@functools.lru_cache(maxsize=None)
def staging_want(nreads, k):
    reads, quals = staging_reads(nreads)
    return oracle(list(reads), list(quals), k)


def masked_block(reads, quals):
    return "_".join("".join(c.lower() if ord(x) < CUT else c.upper() for c, x in zip(r, q)) for r, q in zip(reads, quals))


def pack_reads(reads, quals):
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    out = bytearray()
    for r, q in zip(reads, quals):
        out.extend(code[c.upper()] | (min(ord(x) - 33, 31) << 3) for c, x in zip(r, q))
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


@pytest.mark.parametrize("k,tuning", [(21, SIX), (21, None), (51, None)], ids=["k21-six-byte", "k21-default", "k51"])
@pytest.mark.parametrize("entry", ["reads", "packed", "seq-block"])
def test_staging_through_every_entry_point(k, tuning, entry):
    reads, quals = staging_reads(1500)
    want = staging_want(1500, k)
    b, q, offs = O.reads_to_arrays(list(reads), list(quals))
    with pkg.KmerCounter(k, tuning=tuning) as kc:
        if entry == "reads":
            kc.submit_reads(b, q, offs)
        elif entry == "packed":
            kc.submit_packed_reads(pack_reads(reads, quals), offs)
        else:
            kc.submit_seq_block(masked_block(reads, quals).encode())
        assert_same(kc.sorted_results(), want)
    assert len(want[1]) > 1000


@pytest.mark.parametrize("k,tuning", [(21, SIX), (51, None)], ids=["k21-six-byte", "k51"])
@pytest.mark.parametrize("shift", range(16))
def test_staging_at_every_alignment(k, tuning, shift):
    """device-resident arrays whose first byte lies `shift` bytes behind a 16-byte boundary: qualities aligned like the bases,
    and aligned differently (the instantiation that loads them byte by byte); the packed bytes and the block the same way"""
    import torch
    reads, quals = staging_reads(500)
    want = staging_want(500, k)
    b, q, offs = O.reads_to_arrays(list(reads), list(quals))
    doff = torch.from_numpy(offs.astype(np.int64)).cuda()

    def shifted(a, s):
        d = torch.zeros(len(a) + 64, dtype=torch.uint8, device="cuda")
        d[s:s + len(a)] = torch.from_numpy(a).cuda()
        return d[s:]

    for shift_q in (shift, (shift + 9) % 16):
        db, dq = shifted(b, shift), shifted(q, shift_q)
        torch.cuda.synchronize()
        with pkg.KmerCounter(k, tuning=tuning) as kc:
            kc.submit_reads(db, dq, doff, nreads=len(reads))
            assert_same(kc.sorted_results(), want)
    dp = shifted(pack_reads(reads, quals), shift)
    torch.cuda.synchronize()
    with pkg.KmerCounter(k, tuning=tuning) as kc:
        kc.submit_packed_reads(dp, doff, nreads=len(reads))
        assert_same(kc.sorted_results(), want)
    block = np.frombuffer(masked_block(reads, quals).encode(), dtype=np.uint8).copy()
    dblock = shifted(block, shift)
    torch.cuda.synchronize()
    with pkg.KmerCounter(k, tuning=tuning) as kc:
        kc.submit_seq_block(dblock, length=len(block))
        assert_same(kc.sorted_results(), want)


@pytest.mark.parametrize("k,tuning", [(21, SIX), (51, None)], ids=["k21-six-byte", "k51"])
@pytest.mark.parametrize("where", ["first", "inner", "last"])
def test_a_byte_outside_the_alphabet_is_reported_from_every_position_of_a_group(k, tuning, where):
    """device-resident data at a 16-byte boundary, a whole number of groups long: one byte outside the alphabet at each of the
    sixteen positions of the first, an inner and the last group -> KC_ERR_BAD_BASE, through the three entry points; the
    untouched data passes"""
    import torch
    rng = np.random.default_rng(11)
    reads, quals = random_reads(rng, 60, min_len=60, max_len=120, genome_len=1500, n_rate=0.01)
    cut = sum(len(r) for r in reads) % 16
    reads[-1], quals[-1] = reads[-1][:len(reads[-1]) - cut], quals[-1][:len(quals[-1]) - cut]
    b, q, offs = O.reads_to_arrays(reads, quals)
    assert len(b) % 16 == 0
    block = np.frombuffer(masked_block(reads, quals).encode(), dtype=np.uint8).copy()
    block = block[:len(block) // 16 * 16].copy()
    packed = pack_reads(reads, quals)
    doff = torch.from_numpy(offs.astype(np.int64)).cuda()

    def run(entry, data):
        d = torch.from_numpy(data).cuda()
        assert d.data_ptr() % 16 == 0
        with pkg.KmerCounter(k, tuning=tuning) as kc:
            if entry == "reads":
                kc.submit_reads(d, torch.from_numpy(q).cuda(), doff, nreads=len(reads))
            elif entry == "packed":
                kc.submit_packed_reads(d, doff, nreads=len(reads))
            else:
                kc.submit_seq_block(d, length=len(data))
            kc.results()

    for entry, data in (("reads", b), ("packed", packed), ("seq-block", block)):
        run(entry, data)  # clean
        g0 = {"first": 0, "inner": (len(data) // 32) * 16, "last": len(data) - 16}[where]
        others = [0x40, 0x00, 0xC1, 0x4D, 0x55, 0x0A, 0x7F, 0x5B] + ([0x5F] if entry == "reads" else [])
        for i in range(16):
            bad = data.copy()
            bad[g0 + i] = (bad[g0 + i] & 0xF8) | (5 + i % 3) if entry == "packed" else others[i % len(others)]
            with pytest.raises(pkg.KcError) as e:
                run(entry, bad)
            assert e.value.status == BAD_BASE, (entry, where, i)


# ---- copy-out ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def copy_out_input(kind):
    rng = np.random.default_rng(707)
    reads, quals = random_reads(rng, 3000, min_len=40, max_len=160, genome_len=8000, err=0.005, n_rate=0.002)
    if kind == "hot":
        # one k-mer (and so one level-1 bucket) with some 25 000 occurrences, spread evenly over the input: about 1400 of them
        # in every super-tile of 16384 positions, against the 16 or so of any other bucket
        for i in range(0, 3000, 15):
            reads[i], quals[i] = "A" * 150, "I" * 150
    return tuple(reads), tuple(quals)


@functools.lru_cache(maxsize=None)
def copy_out_want(kind):
    reads, quals = copy_out_input(kind)
    return oracle(list(reads), list(quals), 21)


# k = 21 with 1024 level-1 buckets (six-byte records) and ONE writer: the input's 300 000 positions are some nineteen super-tiles,
# i.e. nineteen rounds of the one workgroup, each adding about sixteen records to every bucket's chain (about 290 a chain in all,
# less per shard in the shard flows).  With a writer per CU (the default) every chain would see one round, starting at its
# beginning, and every run would be simple whatever the chunk size.
SUPER_SPAN = 16384
COPY_OUT = {
    # sixteen-record chunks: from the second round on a run starts inside the chain's last chunk and runs on into new ones
    # (room for 64 x 16 records a chain: nothing overflows) -- the general path in nearly every trip
    "slow-often": ("plain", dict(writers=1, p1=1024, p2=64, chunk1=16, chain1_max=64, ovf_capacity=1 << 20)),
    # a writer per CU and the chunks that go with it: every chain gets one round at its beginning, every run is simple
    "fast-only": ("plain", dict(p1=1024, p2=1024)),
    # chains of three sixteen-record chunks: 48 records a chain, full after the third round or so; the rest of every bucket goes
    # to the overflow list, whose regions the global-table kernels take (kc_flagged_to_table_kernel runs only then)
    "overflow": ("plain", dict(writers=1, p1=1024, p2=64, chunk1=16, chain1_max=3, ovf_capacity=1 << 20)),
    # 512-record chunks: the hot bucket's run of about 1400 starts inside its chain's last chunk and crosses into new ones in every
    # round, while no other chain ever leaves its first chunk -- simple and other runs in one round, and at the hot run's two ends
    # in one wave
    "mixed": ("hot", dict(writers=1, p1=1024, p2=1024, chunk1=512, chain1_max=64)),
}


def merged(parts):
    keys = np.concatenate([p[0] for p in parts])
    order = np.lexsort([keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)])
    return tuple(np.concatenate([p[i] for p in parts])[order] for i in range(4))


@pytest.mark.parametrize("flow", ["plain", "records", "wire-units", "shards-2", "shards-3"])
@pytest.mark.parametrize("case", list(COPY_OUT))
def test_copy_out_paths(case, flow):
    import torch
    k = 21
    kind, tuning = COPY_OUT[case]
    reads, quals = (list(x) for x in copy_out_input(kind))
    want = copy_out_want(kind)
    n = len(reads)
    occ = sum(max(0, len(r) - k - 1) for r in reads)
    assert sum(len(r) for r in reads) > 15 * SUPER_SPAN  # rounds of the one writer
    tuning = dict(tuning)
    if flow == "plain":  # kc_l1_reads16_kernel, two launches (the second continues the chains of the first)
        with pkg.KmerCounter(k, tuning=tuning, time_kernels=True) as kc:
            for a, z in ((0, n // 3), (n // 3, n)):
                kc.submit_reads(*O.reads_to_arrays(reads[a:z], quals[a:z]))
            got = kc.sorted_results()
            times = [kc.kernel_times()]
    elif flow in ("records", "wire-units"):  # kc_l1_records16_kernel / kc_l1_wire6_kernel
        R, wu = 2, flow == "wire-units"
        shards = [pkg.KmerCounter(k, rank_me=r, rank_n=R, tuning=tuning, wire_units=wu, time_kernels=True) for r in range(R)]
        uw, ur, Q = shards[0].wire_unit()
        seg = occ // ur + 8192
        recs = torch.zeros(R * Q * seg * uw, dtype=torch.int64, device="cuda")
        for piece in range(3):
            part = slice(piece * n // 3, (piece + 1) * n // 3)
            counts = shards[piece % R].extract_partition(*O.reads_to_arrays(reads[part], quals[part]), recs, seg)
            for j in range(R * Q):
                if int(counts[j]):
                    shards[j // Q].insert_records(recs[j * seg * uw:], int(counts[j]))
            for d in range(R):
                shards[d].flush()
        got = merged([s.sorted_results() for s in shards])
        times = [s.kernel_times() for s in shards]
        for s in shards:
            s.close()
    else:  # the single-pass shard flow: kc_l1_reads16_kernel<.., true, ..> of every shard on this one GPU
        R = int(flow[-1])
        shards = [pkg.KmerCounter(k, rank_me=r, rank_n=R, tuning=tuning, time_kernels=True) for r in range(R)]
        seg_words = occ * shards[0].rec_nl + 4096
        segs = torch.zeros(R * seg_words, dtype=torch.int64, device="cuda")
        for r in range(R):
            mine = list(range(r, n, R))
            words = shards[r].shard_extract(*O.reads_to_arrays([reads[i] for i in mine], [quals[i] for i in mine]), segs, seg_words)
            for d in range(R):
                w = int(words[d])
                if d != r and w:
                    dst = shards[d].shard_reserve(w)
                    dst.copy_(segs[d * seg_words:d * seg_words + w])
                    torch.cuda.synchronize()
                    shards[d].shard_commit(dst, w)
        got = merged([s.sorted_results() for s in shards])
        times = [s.kernel_times() for s in shards]
        for s in shards:
            s.close()
    assert_same(got, want)
    assert len(want[1]) > 5000
    # the overflow case overflows (and the sixteen-record case that must not, does not: its general-path trips are straddles)
    fallback = sum(t.get("kc_flagged_to_table_kernel", (0, 0.0))[0] for t in times)
    if case == "overflow":
        assert fallback > 0
    if case == "slow-often":
        assert fallback == 0
