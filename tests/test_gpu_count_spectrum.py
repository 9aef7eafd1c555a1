"""kc_count_spectrum on the device: the histogram of the results' counts equals numpy's of the oracle's, and the counts a
construction fixes land in their bins on both sides of every boundary the kernel has."""
import ctypes as C

import numpy as np
import pytest
import torch

import count_cases as CC
import kdepth_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from oracle import cpu_oracle as O
from test_gpu_kmer_depths import case, counter

pytestmark = pytest.mark.gpu

LOW = 1024  # SPECT_LOW of csrc/kc_kdepth.hpp: counts below it go to a workgroup's LDS bins, the others to global atomics


def spectrum_of(kc, want_counts):
    """count_spectrum both ways, held to the model of the counts that are expected"""
    want, wst = M.spectrum(want_counts)
    hist, st = kc.count_spectrum()
    dhist, dst = kc.count_spectrum(on_device=True)
    assert hist.dtype == np.uint64 and dhist.dtype == torch.int64 and dhist.is_cuda and len(hist) == len(dhist) == M.BINS
    assert (hist == want).all() and (dhist.cpu().numpy().view(np.uint64) == want).all(), np.flatnonzero(hist != want)[:10]
    assert st == wst == dst
    ks = kc.stats()
    assert (st["kmers"], st["sum_counts"]) == (ks["total_kmers"], ks["sum_counts"])
    assert pkg.format_spectrum(hist) == M.format_spectrum(want) == pkg.format_spectrum(dhist)
    return hist, st


@pytest.mark.parametrize("k", (21, 33, 99))
def test_random_reads_equal_the_oracle(k):
    counts = case(k)[2][1]
    with counter(k) as kc:
        hist, st = spectrum_of(kc, counts)
    assert st["kmers"] == len(counts) > 1000 and np.count_nonzero(hist) > 5


@pytest.mark.parametrize("m", sorted({2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, LOW - 1, LOW, LOW + 1}))
def test_every_result_at_one_count(m):
    """m identical reads of a repeat-free genome: all but its two end k-mers survive with count m, so one bin takes them all,
    the worst case of the LDS atomics below LOW and of one global address from it on"""
    k = 21
    g = M.unique_genome(np.random.default_rng(m), 1500, k)
    b, q, offs = O.reads_to_arrays([g.decode()] * m)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(b, q, offs)
        kc.finalize()
        hist, st = spectrum_of(kc, np.full(len(g) - k - 1, m))
    assert hist[m] == len(g) - k - 1 == st["mode_kmers"] and st["mode_count"] == st["max_count"] == m


def test_a_spread_of_counts_across_the_lds_range():
    k, dmin = 21, 2
    pick = CC.KmerPicker(k, 11)
    cases = [CC.Case("n=%d" % n, pick(), [[(("A", "C"), n)]]) for n in range(2, 2050)]
    b, q, offs = CC.emit(cases, k, seed=5, shuffle=False)
    want = CC.expected_results(cases, dmin)[1]
    assert len(np.unique(want)) == 2048
    with pkg.KmerCounter(k, dmin_thres=dmin) as kc:
        kc.submit_reads(b, q, offs)
        kc.finalize()
        hist, st = spectrum_of(kc, want)
    assert st["max_count"] == 2049 and st["mode_count"] == 2 and st["mode_kmers"] == 1  # a tie of all: the smallest count


def test_saturated_counts():
    k, dmin = 21, 2
    cases = CC.saturation(k)
    b, q, offs = CC.emit(cases, k, seed=6, shuffle=False)
    want = CC.expected_results(cases, dmin)[1]
    assert (want == 65535).sum() >= 2 and (want < 65535).any()
    with pkg.KmerCounter(k, dmin_thres=dmin) as kc:
        kc.submit_reads(b, q, offs)
        kc.finalize()
        hist, st = spectrum_of(kc, want)
    assert st["saturated"] == int((want == 65535).sum()) == hist[65535] and st["max_count"] == 65535


def test_no_results_and_the_arguments():
    with pkg.KmerCounter(21) as kc:
        kc.finalize()
        hist, st = spectrum_of(kc, np.zeros(0, np.uint16))
        assert not hist.any() and st == dict.fromkeys(M.SPECTRUM_STATS, 0)
    k = 21
    with counter(k) as kc:  # either output alone
        want, wst = M.spectrum(case(k)[2][1])
        L = pkg.lib()
        st = pkg._lib.kc_spectrum_stats()
        hist = np.zeros(M.BINS, np.uint64)
        assert L.kc_count_spectrum(kc._h, None, 0, C.byref(st)) == 0 and L.kc_count_spectrum(kc._h, None, 1, C.byref(st)) == 0
        assert {n: getattr(st, n) for n in M.SPECTRUM_STATS} == wst
        assert L.kc_count_spectrum(kc._h, hist.ctypes.data, 0, None) == 0 and (hist == want).all()
        assert L.kc_count_spectrum(kc._h, None, 0, None) == pkg._lib.KC_ERR_INVALID_ARG and b"both NULL" in L.kc_last_error()
