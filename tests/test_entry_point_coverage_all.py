"""Every function include/kcount_mi355.h declares has a place in the poisoned-scratch tests ("Poisoned scratch") or
a reason not to.  tests/test_poisoned_scratch_coverage.py finds entry points in csrc/ by the text of their linkage specifier;
an entry point that takes its C linkage from the header's declaration alone (csrc/kc_api_kdepth.hpp) does not show there.
This guard reads the header -- the parse tests/test_abi.py holds the exports and the binding to -- so no entry point arrives
unlisted, however it is spelled.  No GPU is needed: the header and the test modules are read as text."""
import os
import re

from test_abi import header_functions
from test_poisoned_scratch_coverage import COVERED as OLD_COVERED
from test_poisoned_scratch_coverage import EXEMPT as OLD_EXEMPT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KDEPTH = "test_gpu_poisoned_scratch_kdepth"

# entry point -> (module, test), for what the older guard's lists do not hold
COVERED = {
    "kc_seq_kmer_depths": (KDEPTH, "test_kmer_depths_equal_the_model"),
    "kc_count_spectrum": (KDEPTH, "test_count_spectrum_equals_the_model"),
}
# the wrapper of kcount.py a test goes through
WRAPPERS = {"kc_seq_kmer_depths": ".kmer_depths(", "kc_count_spectrum": ".count_spectrum("}
EXEMPT = {}


def test_every_declared_function_is_covered_or_exempt():
    names = set(header_functions())
    assert len(names) >= 72 and {"kc_seq_kmer_depths", "kc_count_spectrum", "kc_create"} <= names
    lists = (OLD_COVERED, OLD_EXEMPT, COVERED, EXEMPT)
    assert sum(len(x) for x in lists) == len(set().union(*lists)), "a name in two lists"
    missing = sorted(names - set().union(*lists))
    assert not missing, "declared in the header without a poisoned-scratch test or a reason: %s" % missing
    stale = sorted((set(COVERED) | set(EXEMPT)) - names)
    assert not stale, "listed here, but not declared in the header: %s" % stale
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())


def test_the_covering_tests_exist_set_the_fill_and_call_the_entry_point():
    body = {}
    for name, (module, test) in COVERED.items():
        if module not in body:
            src = open(os.path.join(ROOT, "tests", module + ".py")).read()
            assert "pytestmark = pytest.mark.gpu" in src and 'monkeypatch.setenv("KC_DEBUG_FILL"' in src and "kc_debug_filled_bytes()" in src, module
            body[module] = dict(re.findall(r"^def (test_\w+)\((.*?)(?=^def |^# ----|\Z)", src, flags=re.S | re.M))
        assert test in body[module], "%s: no test %s in %s" % (name, test, module)
        text = body[module][test]
        assert text.startswith("fill"), "%s::%s does not take the fill fixture" % (module, test)
        assert WRAPPERS[name] in text or name in text, "%s::%s does not call %s" % (module, test, name)
