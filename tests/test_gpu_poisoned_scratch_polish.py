"""kc_ctg_polish on memory that is not zero when the library gets it: KC_DEBUG_FILL fills every fresh allocation of the
library ("Poisoned scratch"), 0xA5 and 0x5A a case, and the call still equals tests/polish_model.py exactly.  The
statistics, the contigs' accumulators, the best records, the keys and the permutation's two buffers, the sort's counters, the
lanes' and tiles' numbers of changed columns, their scanned bases, and a host caller's staged reads, records, block, counts
and fixes are all fresh allocations of a call.  Contexts are made after the variable is set, and every test checks that
kc_debug_filled_bytes() rose.  Beside the ordinary cases: a larger call followed by a smaller one on the same context."""
import pytest

import polish_cases as PC
import mhm2_kmer_analysis_v2_amd as pkg
from test_gpu_polish import args, call, counter, same

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
SIDES = pytest.mark.parametrize("device", (True, False), ids=("device", "host"))


@pytest.fixture(params=FILLS, ids=["0xA5", "0x5A"])
def fill(request, monkeypatch):
    monkeypatch.setenv("KC_DEBUG_FILL", "0x%02X" % request.param)
    before = pkg.lib().kc_debug_filled_bytes()
    yield request.param
    assert pkg.lib().kc_debug_filled_bytes() > before, "nothing was filled: the test proves nothing"


@SIDES
@pytest.mark.parametrize("name", ("tiles", "strands", "classes", "empty"))
def test_polish_equals_the_model(fill, name, device):
    c = PC.case(name)
    with counter(c) as kc:
        same(call(kc, c, device), PC.expected(name))
        a, q = args(c, device)
        same(kc.polish_contigs(*a, quals=q, with_fixes=False, with_records=False, **c.kw), PC.expected(name), counts=False, records=False, fixes=False)


@SIDES
def test_polish_larger_then_smaller(fill, device):
    big, small = PC.case("long"), PC.case("columns")
    with counter(big) as kc:
        for _ in range(2):
            same(call(kc, big, device), PC.expected("long"))
            kc.index_contigs(*small.contig_block())
            same(call(kc, small, device), PC.expected("columns"))
            kc.index_contigs(*big.contig_block())
