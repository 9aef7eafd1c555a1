"""Level 2 of six-byte level-1 records (kc_l2_rec6_kernel) in rounds of two half-rounds: a region's run of a round comes
from both halves, is staged as 32-bit words in two sorted parts and copied out in region order.  Runs far longer than
32 records per region and round, chains of 16-record chunks so that a run crosses many chunks, chains that fill up
inside a run, and instalments that stop in the middle of a chain -- all against the oracle, bit-exact."""
import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
from helpers import random_reads
from oracle import cpu_oracle as O

pytestmark = pytest.mark.gpu


def _case(k, seed, nreads, genome_len):
    rng = np.random.default_rng(seed)
    reads, quals = random_reads(rng, nreads, min_len=k + 2, max_len=k + 140, genome_len=genome_len, err=0.01, n_rate=0.002)
    b, q, offs = O.reads_to_arrays(reads, quals)
    o = O.Oracle(k, nranks=4, nthreads=8)
    o.add_reads(b, q, offs)
    table = o.dump_table()
    want = o.finalize()
    st = o.stats()
    o.close()
    assert st["dropped"] == 0
    return reads, quals, want, table, st


def _check(got, gtable, gst, want, wtable, wst):
    for g, w in zip(got, want):
        assert g.shape == w.shape and (g == w).all()
    assert all((gtable[i] == wtable[i]).all() for i in range(3))
    assert gst["num_unique"] == wst["unique"] and gst["sum_counts"] == wst["sum_counts"]
    assert gst["kmers_inserted"] == wst["kmers_inserted"]


# (k, tuning): every one makes level 1 write six-byte records (compact, 2k - log2 P1 <= 32)
LONG_RUNS = {
    # two regions per bucket: runs of thousands of records per round, three rounds and an odd tail per bucket
    "two-regions": (13, dict(writers=3, p1=2, p2=2, slots=4096, chunk1=16, chunk2=16)),
    # one wave's worth of regions, and two
    "64-regions": (17, dict(writers=2, p1=4, p2=64, slots=2048, chunk2=16)),
    "128-regions-odd-writers": (17, dict(writers=5, p1=8, p2=128, slots=1024, chunk1=32, chunk2=32)),
    # chains that fill up inside a run: the rest of the run goes to the region overflow list (and that list grows)
    "chains-fill-up": (13, dict(writers=2, p1=2, p2=4, slots=4096, chunk2=16, chain2_max=10, ovf_capacity=20000)),
    # the benchmark's fan-outs
    "1024x1024": (21, dict(p1=1024, p2=1024)),
}


@pytest.mark.parametrize("case", list(LONG_RUNS))
def test_long_runs_across_chunks_match_oracle(case):
    k, tuning = LONG_RUNS[case]
    reads, quals, want, wtable, wst = _case(k, 700 + k, 4000, 6000)
    with pkg.KmerCounter(k, tuning=tuning, time_kernels=True) as kc:
        for a, z in ((0, 1), (1, 1777), (1777, 4000)):  # chains continue a partly filled last chunk in later launches
            b, q, o = O.reads_to_arrays(reads[a:z], quals[a:z])
            kc.submit_reads(b, q, o)
        gtable = kc.dump_table()
        got = kc.sorted_results()
        st = kc.stats()
        kt = kc.kernel_times()
    _check(got, gtable, st, want, wtable, wst)
    assert kt.get("kc_l2_rec6_kernel", (0, 0.0))[0] >= 1, kt


@pytest.mark.parametrize("k,tuning", [
    (13, dict(writers=3, p1=2, p2=8, slots=4096, chunk1=16, chunk2=16)),
    (17, dict(writers=2, p1=4, p2=64, slots=2048, chunk2=16, chain2_max=40, ovf_capacity=1 << 20)),
], ids=["k13-few-regions", "k17-short-chains"])
def test_instalments_that_stop_mid_chain(monkeypatch, k, tuning):
    """The host pipe's level 2 between blocks takes what has arrived -- a chain's records up to wherever a block ended,
    an odd number as often as not -- and the next instalment starts behind them; a small buffer hands level 1 on to
    level 2 the same way (bk_light_spill)."""
    reads, quals, want, wtable, wst = _case(k, 900 + k, 6000, 8000)
    b, q, o = O.reads_to_arrays(reads, quals)
    monkeypatch.setenv("KC_HOST_BLOCK", str(1 << 16))  # bytes of bases per block: about a dozen blocks
    monkeypatch.setenv("KC_L2_INSTALMENTS", "1")
    for cap in (None, int(wst["kmers_inserted"]) // 3):
        kw = {} if cap is None else dict(max_kmers_buffered=cap)
        with pkg.KmerCounter(k, tuning=tuning, time_kernels=True, **kw) as kc:
            kc.submit_reads(b, q, o)
            gtable = kc.dump_table()
            got = kc.sorted_results()
            st = kc.stats()
            kt = kc.kernel_times()
        _check(got, gtable, st, want, wtable, wst)
        assert kt.get("kc_l2_rec6_kernel", (0, 0.0))[0] >= 3, kt
