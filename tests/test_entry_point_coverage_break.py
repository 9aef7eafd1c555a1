"""include/kcount_mi355_break.h, the fourth public header, held to the rule tests/test_abi.py and
tests/test_entry_point_coverage_all.py hold the first to, tests/test_entry_point_coverage_correct.py the second and
tests/test_entry_point_coverage_polish.py the third: every function it declares is exported by the library, bound in
_lib.SYMBOLS_BREAK with the declaration's number of arguments, and covered by a named test of a gpu module that sets
KC_DEBUG_FILL, reads kc_debug_filled_bytes() and takes the fill fixture ("Poisoned scratch").  The four headers and
the four symbol tables share no name.  No GPU is needed: the headers and the test modules are read as text."""
import os
import re

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib
from test_abi import header_functions as first_header_functions
from test_entry_point_coverage_correct import header_functions as second_header_functions
from test_entry_point_coverage_polish import header_functions as third_header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kcount_mi355_break.h")

BREAK = "test_gpu_poisoned_scratch_break"
# entry point -> (module, test)
COVERED = {"kc_ctg_break": (BREAK, "test_break_equals_the_model")}
# the wrapper of kcount.py a test goes through
WRAPPERS = {"kc_ctg_break": ".break_contigs("}
EXEMPT = {}


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_functions():
    return sorted(set(re.findall(r"\b(kc_[a-z_0-9]+)\s*\(", header_source())))


def test_the_fourth_header_builds_on_the_first_and_the_four_share_no_name():
    src = header_source()
    assert '#include "kcount_mi355.h"' in src and src.count('extern "C" {') == 1
    names = header_functions()
    assert names == ["kc_ctg_break"]
    headers = [set(first_header_functions()), set(second_header_functions()), set(third_header_functions()), set(names)]
    tables = [set(_lib.SYMBOLS), set(_lib.SYMBOLS_CORRECT), set(_lib.SYMBOLS_POLISH), set(_lib.SYMBOLS_BREAK)]
    for group in (headers, tables):
        assert all(group) and sum(len(g) for g in group) == len(set().union(*group))
    assert [sorted(h) for h in headers[1:]] == [sorted(t) for t in tables[1:]]


def test_the_definition_has_no_linkage_specifier_of_its_own():
    src = open(os.path.join(ROOT, "mhm2_kmer_analysis_v2_amd", "csrc", "kc_api_break.hpp")).read()
    code = re.sub(r"//.*", "", src)
    assert re.search(r"^int kc_ctg_break\(", code, flags=re.M) and 'extern "C"' not in code


def test_library_exports_and_binds_every_declared_symbol():
    L = pkg.lib()
    names = header_functions()
    src = header_source()
    for n in names:
        assert hasattr(L, n), "libkcount_mi355.so does not export %s" % n
        assert n in _lib.SYMBOLS_BREAK, "python binding lacks %s" % n
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, src, flags=re.S).group(1)
        res, args = _lib.SYMBOLS_BREAK[n]
        assert len(args) == params.count(",") + 1 and getattr(L, n).argtypes == args and getattr(L, n).restype is res
    assert sorted(_lib.SYMBOLS_BREAK) == names


def test_every_declared_function_is_covered_or_exempt():
    names = set(header_functions())
    assert not set(COVERED) & set(EXEMPT)
    missing = sorted(names - set(COVERED) - set(EXEMPT))
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
