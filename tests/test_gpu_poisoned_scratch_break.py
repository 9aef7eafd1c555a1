"""kc_ctg_break on memory that is not zero when the library gets it: KC_DEBUG_FILL fills every fresh allocation of the
library ("Poisoned scratch"), 0xA5 and 0x5A a case, and the call still equals tests/break_model.py exactly.  The
statistics, the two difference arrays, the weak flags, the tiles' sums, maxima and break counts, the breaks' ranks and a host
caller's staged offsets, records, pairs, depths and outputs are all fresh allocations of a call.  Contexts are made after the
variable is set, and every test checks that kc_debug_filled_bytes() rose.  Beside the ordinary cases: a larger call followed by
a smaller one on the same context."""
import pytest

import break_cases as BC
import mhm2_kmer_analysis_v2_amd as pkg
from test_gpu_ctg_break import args, call, counter, same

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
@pytest.mark.parametrize("name", ("size_t+1", "cut_tile_first", "classes", "gather17", "none"))
def test_break_equals_the_model(fill, name, device):
    c = BC.case(name)
    with counter(c) as kc:
        same(call(kc, c, device), BC.expected(name))
        a, _ = args(c, device, depths=False)
        same(kc.break_contigs(*a, **c.kw), BC.expected(name), depths=False, tracks=False)


@SIDES
def test_break_larger_then_smaller(fill, device):
    big, small = BC.case("gather4097"), BC.case("margins")
    with counter(big) as kc:
        for _ in range(2):
            same(call(kc, big, device), BC.expected("gather4097"))
            kc.index_contigs(*small.contig_block())
            same(call(kc, small, device), BC.expected("margins"))
            kc.index_contigs(*big.contig_block())
