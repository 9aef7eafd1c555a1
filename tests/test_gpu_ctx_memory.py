"""A context's device memory: kc_destroy gives back what create, the submits, the contig pass, the dumps, lookups, sorts,
resets and the read front end took (sixteen whole lives of a context leave the device's free memory where it was), and
an ordinary error return leaves the context able to count.  Everything a cycle computes is compared with the oracle or
the front end's models, so a cycle that ran nothing cannot pass.  No tolerances."""
import functools
import os

import numpy as np
import pytest

import merge_model as MM
import mhm2_kmer_analysis_v2_amd as pkg
import trim_model as TM
from mhm2_kmer_analysis_v2_amd import _lib
from helpers import random_reads
from oracle import cpu_oracle as O
from test_gpu_parity import arrays, assert_same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FA_PATH = os.path.join(HERE, "golden", "adapters_no_transposase.fa")
KS = (21, 31, 63)  # 31 and 63: the library's record is one word wider than the reference's key
MIN_TABLE_BYTES = 32 << 20
# max_kmers_buffered.  A process pays once for the first use of every kernel family (code, scratch, queues: 149 MB over the
# three k here when nothing ran before, less after other tests), which is no leak but lies between the two readings; so the
# arenas are sized for the smallest table_bytes of a cycle (373 MB, k = 21) to exceed that, and a block of a context's that
# is lost once a cycle still shows sixteen-fold
BUFFERED = 1 << 24


@functools.lru_cache(maxsize=None)
def cycle_reads():
    reads, quals = random_reads(np.random.default_rng(1605), 2000, min_len=100, max_len=100, genome_len=6000)
    ctg_rng = np.random.default_rng(1606)
    genome = "".join(ctg_rng.choice(list("ACGT"), size=3000))
    ctgs = [genome[a:a + 400] for a in range(0, 2600, 300)] + [reads[0].replace("N", "A"), reads[1].replace("N", "C")]
    depths = [3 + 2 * i for i in range(len(ctgs))]
    return reads, quals, ctgs, depths


@functools.lru_cache(maxsize=None)
def cycle_oracle(k):
    """(pre-purge dump, results with the contigs, results of the reads alone) for the cycle's reads at k"""
    reads, quals, ctgs, depths = cycle_reads()
    b, q, offs = arrays(reads, quals)
    o = O.Oracle(k, nranks=2, nthreads=2)
    o.add_reads(b, q, offs)
    plain = o.finalize()
    o.close()
    o = O.Oracle(k, nranks=2, nthreads=2)
    o.add_reads(b, q, offs)
    table = o.dump_table()
    for c, d in zip(ctgs, depths):
        o.add_ctg(c, d)
    with_ctgs = o.finalize()
    o.close()
    assert len(with_ctgs[1]) > len(plain[1]) > 1000
    return table, with_ctgs, plain


@functools.lru_cache(maxsize=None)
def front_end_case():
    """ten pairs with adapters behind short fragments, and what the models make of them"""
    seqs = TM.read_fasta_seqs(FA_PATH)
    b, q, o = TM.random_pairs(1607, 10, seqs)
    ads = TM.AdapterSet(open(FA_PATH, "rb").read(), 21, False)
    return (b, q, o), TM.trim_reads(ads, b, q, o, True), MM.merge_pairs(b, q, o, 33, 21)


def masked_block(reads, quals):
    """kc_submit_seq_block's input: the reads joined by '_', a base of quality below 20 in lower case"""
    return "_".join("".join(c.lower() if ord(x) < 33 + 20 else c for c, x in zip(r, ql)) for r, ql in zip(reads, quals)).encode()


def device_lookup(kc, keys):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).cuda()
    n = len(keys)
    dc = torch.zeros(n, dtype=torch.int16, device="cuda")
    dl, dr = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(pkg.lib().kc_lookup(kc._h, dq.data_ptr(), n, 1, dc.data_ptr(), dl.data_ptr(), dr.data_ptr()), "kc_lookup")
    kc.flush()  # the stream has run the lookup
    return dc.cpu().numpy().view(np.uint16), dl.cpu().numpy(), dr.cpu().numpy()


def one_cycle(k, k_next, dev_reads):
    """One life of a context; returns its table_bytes."""
    reads, quals, ctgs, depths = cycle_reads()
    wtable, want, _ = cycle_oracle(k)
    third = len(reads) // 3
    with pkg.KmerCounter(k, max_kmers_buffered=BUFFERED, time_kernels=True) as kc:
        kc.submit_reads(*arrays(reads[:third], quals[:third]))  # host arrays: the host pipe
        kc.submit_reads(*dev_reads, nreads=third)  # reads [third, 2 * third) as device tensors
        kc.submit_seq_block(masked_block(reads[2 * third:], quals[2 * third:]))
        kc.begin_ctg_kmers(sum(len(c) for c in ctgs))
        half = len(ctgs) // 2
        kc.submit_ctgs(ctgs[:half], depths[:half])
        kc.submit_ctgs(ctgs[half:], depths[half:])
        gtable = kc.dump_table()
        assert all((g == w).all() for g, w in zip(gtable, wtable))
        got = kc.sorted_results()
        assert_same(got, want)
        table_bytes = kc.stats()["table_bytes"]
        for look in (kc.lookup, functools.partial(device_lookup, kc)):
            cnt, left, right = look(want[0][::5])
            assert (cnt == want[1][::5]).all() and (left == want[2][::5]).all() and (right == want[3][::5]).all()
        kc.sort_results()
        assert_same(kc.results(), want)  # in key order without the host's sort
        assert kc.kernel_times()
        kc.reset(k_next)
        kc.submit_reads(*arrays(reads, quals))
        assert_same(kc.sorted_results(), cycle_oracle(k_next)[2])
        (b, q, o), wtrim, wmerge = front_end_case()
        kc.load_adapters(FA_PATH, 21)
        tb, tq, to, tst = kc.trim_adapters(b, q, o, paired=True)
        assert tst == wtrim[3] and np.array_equal(to.cpu().numpy().view(np.uint64), np.asarray(wtrim[2], dtype=np.uint64))
        assert np.array_equal(tb.cpu().numpy(), wtrim[0]) and np.array_equal(tq.cpu().numpy(), wtrim[1])
        packed, mo, mst = kc.merge_pairs(b, q, o, min_kmer_len=21)
        assert np.array_equal(packed.cpu().numpy(), wmerge[0]) and np.array_equal(mo.cpu().numpy().view(np.uint64), np.asarray(wmerge[1], dtype=np.uint64))
        assert all(mst[s] == wmerge[2][s] for s in ("pairs", "merged", "out_reads", "out_bases"))
    return table_bytes


def test_destroy_gives_back_what_a_context_took():
    import torch
    reads, quals, _, _ = cycle_reads()
    third = len(reads) // 3
    b, q, offs = arrays(reads[third:2 * third], quals[third:2 * third])
    dev_reads = (torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda())
    for k in KS:
        cycle_oracle(k)
    front_end_case()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # torch's own cache is not the library's
    free_before = torch.cuda.mem_get_info()[0]
    table_bytes = [one_cycle(KS[i % 3], KS[(i + 1) % 3], dev_reads) for i in range(16)]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free_after = torch.cuda.mem_get_info()[0]
    print("free device memory: %d before, %d after (drop %d); table_bytes per cycle %d .. %d" % (
        free_before, free_after, free_before - free_after, min(table_bytes), max(table_bytes)))
    assert min(table_bytes) >= MIN_TABLE_BYTES
    assert free_before - free_after < min(table_bytes)


def test_error_returns_leave_the_context_usable():
    import torch
    rng = np.random.default_rng(1608)
    reads, quals = random_reads(rng, 300, min_len=40, max_len=120, genome_len=1500)
    b, q, offs = arrays(reads, quals)
    ctg = "".join(rng.choice(list("ACGT"), size=6000))  # ~6000 distinct k-mers
    want = {}
    for k in (21, 33):
        o = O.Oracle(k, nranks=2, nthreads=1)
        o.add_reads(b, q, offs)
        want[k] = o.finalize()
        o.close()
    o = O.Oracle(21, nranks=2, nthreads=1)
    o.add_reads(b, q, offs)
    o.add_ctg(ctg, 5)
    want_ctg = o.finalize()
    o.close()
    assert len(want_ctg[1]) > len(want[21][1]) + 5000

    def bad_character(kc):
        kc.submit_reads(b, q, offs)
        kc.begin_ctg_kmers(1000)
        kc.submit_ctgs(["ACGTX"], [5])  # shorter than a k-mer: nothing of it is in the contig table

    def lookup_before_finalize(kc):
        kc.submit_reads(b, q, offs)
        keys = np.zeros((4, kc.nl), dtype=np.uint64)
        cnt = np.zeros(4, dtype=np.uint16)
        _lib.check(pkg.lib().kc_lookup(kc._h, keys.ctypes.data, 4, 0, cnt.ctypes.data, None, None), "kc_lookup")

    def insert_after_finalize(kc):
        kc.submit_reads(b, q, offs)
        kc.finalize()
        kc.insert_records(torch.zeros(64 * kc.rec_nl, dtype=torch.int64, device="cuda"), 64)

    def small_contig_table(kc):
        kc.submit_reads(b, q, offs)
        kc.begin_ctg_kmers(10)  # -> 1024 slots
        kc.submit_ctgs([ctg], [5])

    for provoke, status in ((bad_character, -7), (lookup_before_finalize, -8), (insert_after_finalize, -8), (small_contig_table, -6)):
        with pkg.KmerCounter(21) as kc:
            with pytest.raises(pkg.KcError) as e:
                provoke(kc)
            assert e.value.status == status, provoke.__name__
            if provoke is small_contig_table:  # a new contig pass replaces the one that ran out of room
                kc.begin_ctg_kmers(8000)
                kc.submit_ctgs([ctg], [5])
                assert_same(kc.sorted_results(), want_ctg)
            else:
                assert_same(kc.sorted_results(), want[21])
            for k in (33, 21):
                kc.reset(k)
                kc.submit_reads(b, q, offs)
                assert_same(kc.sorted_results(), want[k])
