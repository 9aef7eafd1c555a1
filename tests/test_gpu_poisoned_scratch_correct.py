"""kc_correct_reads on memory that is not zero when the library gets it: KC_DEBUG_FILL fills every fresh allocation of the
library ("Poisoned scratch"), 0xA5 and 0x5A a case, and the call still equals tests/correct_model.py exactly.  The
scratch track, the per-lane and per-workgroup site counts, the per-sequence weak windows, reasons and corrected bytes, a round's
sites, verdicts, slots and fixes, and a host caller's staged text and records are all fresh allocations of a call.  Contexts
are made after the variable is set, and every test checks that kc_debug_filled_bytes() rose.  Beside the ordinary block: a
larger call followed by a smaller one on the same context."""
import pytest

import correct_cases as CC
import correct_model as M
import kdepth_model as K
import mhm2_kmer_analysis_v2_amd as pkg
from test_gpu_correct_reads import counter, counts_of, model, on_device, same

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
SIDES = pytest.mark.parametrize("device", (True, False), ids=("device", "host"))


@pytest.fixture(params=FILLS, ids=["0xA5", "0x5A"])
def fill(request, monkeypatch):
    monkeypatch.setenv("KC_DEBUG_FILL", "0x%02X" % request.param)
    before = pkg.lib().kc_debug_filled_bytes()
    yield request.param
    assert pkg.lib().kc_debug_filled_bytes() > before, "nothing was filled: the test proves nothing"


def args(b, offs, device):
    return on_device(b, offs) if device else (b, offs)


@SIDES
@pytest.mark.parametrize("k", (21, 99))
def test_correct_reads_equal_the_model(fill, k, device):
    b, offs, _ = CC.block(k)
    with counter(k) as kc:
        same(kc.correct_reads(*args(b, offs, device), with_fixes=True), model(k))
        same(kc.correct_reads(*args(b, offs, device), min_windows=1, with_fixes=True), model(k, min_windows=1))
        same(kc.correct_reads(*args(b, offs, device), min_windows=1, with_records=False), model(k, min_windows=1))


@SIDES
def test_correct_reads_larger_then_smaller(fill, device):
    k = 33
    b, offs, _ = CC.block(k)
    small = K.block([c[1] for c in CC.planted_cases(k)[3:9]])
    with counter(k) as kc:
        for _ in range(2):
            same(kc.correct_reads(*args(b, offs, device), with_fixes=True), model(k))
            same(kc.correct_reads(*args(*small, device), with_fixes=True), M.correct_reads(counts_of(k), k, *small))
