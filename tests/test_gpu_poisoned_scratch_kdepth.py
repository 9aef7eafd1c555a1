"""kc_seq_kmer_depths and kc_count_spectrum on memory that is not zero when the library gets it: KC_DEBUG_FILL fills every
fresh allocation of the library ("Poisoned scratch"), 0xA5 and 0x5A a case, and both still equal
tests/kdepth_model.py exactly.  The per-sequence sums, the "none" of the minimum, the statistics words, a host caller's
staged track and records and the histogram's scratch are all fresh allocations of a call.  Contexts are made after the
variable is set, and every test checks that kc_debug_filled_bytes() rose.  Beside the ordinary block: sequences that are
all shorter than k (no item writes a sum), a context without results (no probe finds anything, the histogram kernel does
not run), and a larger call followed by a smaller one on the same context."""
import numpy as np
import pytest

import kdepth_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from test_gpu_kmer_depths import case, counter, mixed_block, model, on_device, same

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
SIDES = pytest.mark.parametrize("device", (True, False), ids=("device", "host"))


@pytest.fixture(params=FILLS, ids=["0xA5", "0x5A"])
def fill(request, monkeypatch):
    monkeypatch.setenv("KC_DEBUG_FILL", "0x%02X" % request.param)
    before = pkg.lib().kc_debug_filled_bytes()
    yield request.param
    assert pkg.lib().kc_debug_filled_bytes() > before, "nothing was filled: the test proves nothing"


def args(sb, offs, device):
    return on_device(sb, offs) if device else (sb, offs)


@SIDES
@pytest.mark.parametrize("k", (21, 64, 99))
def test_kmer_depths_equal_the_model(fill, k, device):
    sb, offs = mixed_block(k)
    with counter(k) as kc:
        for fill_mean in (False, True):
            want = model(k, "mixed", sb, offs, min_count=0, fill_mean=fill_mean)
            same(kc.kmer_depths(*args(sb, offs, device), fill_mean=fill_mean), want)
            same(kc.kmer_depths(*args(sb, offs, device), fill_mean=fill_mean, with_records=False), want)


@SIDES
def test_kmer_depths_where_nothing_is_written(fill, device):
    k = 33
    G, _, _, tab = case(k)
    short = M.block([G[i:i + (i % k)] for i in range(0, 2000, 7)])
    with counter(k) as kc:
        for fill_mean in (False, True):
            want = M.kmer_depths(tab, k, *short, fill_mean=fill_mean)
            assert want[2]["windows"] == 0 and not want[0].any()
            same(kc.kmer_depths(*args(*short, device), fill_mean=fill_mean), want)
    sb, offs = mixed_block(k)
    with pkg.KmerCounter(k) as kc:  # no results
        kc.finalize()
        for fill_mean in (False, True):
            want = M.kmer_depths({}, k, sb, offs, fill_mean=fill_mean)
            same(kc.kmer_depths(*args(sb, offs, device), fill_mean=fill_mean), want)
        hist, st = kc.count_spectrum(on_device=device)
        assert not (hist.cpu().numpy() if device else hist).any() and st == dict.fromkeys(M.SPECTRUM_STATS, 0)


@SIDES
def test_kmer_depths_larger_then_smaller(fill, device):
    k = 21
    sb, offs = mixed_block(k)
    small = M.block([bytes(sb[int(offs[i]):int(offs[i + 1])]) for i in range(12, 16)])
    tab = case(k)[3]
    with counter(k) as kc:
        for fill_mean in (False, True):
            same(kc.kmer_depths(*args(sb, offs, device), fill_mean=fill_mean), model(k, "mixed", sb, offs, min_count=0, fill_mean=fill_mean))
            same(kc.kmer_depths(*args(*small, device), fill_mean=fill_mean), M.kmer_depths(tab, k, *small, fill_mean=fill_mean))


@SIDES
@pytest.mark.parametrize("k", (21, 99))
def test_count_spectrum_equals_the_model(fill, k, device):
    want, wst = M.spectrum(case(k)[2][1])
    with counter(k) as kc:
        for _ in range(2):
            hist, st = kc.count_spectrum(on_device=device)
            assert ((hist.cpu().numpy().view(np.uint64) if device else hist) == want).all() and st == wst
