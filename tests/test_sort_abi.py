"""kc_sort_results and kc_dump_text_device reject a NULL context before they touch a device (no GPU needed)."""
import ctypes as C

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib


def test_sort_results_null_context():
    r = _lib.kc_result()
    assert pkg.lib().kc_sort_results(None, C.byref(r)) == _lib.KC_ERR_INVALID_ARG
    assert pkg.lib().kc_sort_results(None, None) == _lib.KC_ERR_INVALID_ARG


def test_dump_text_device_null_context():
    nb = C.c_uint64(7)
    assert pkg.lib().kc_dump_text_device(None, 0, 0, None, 0, C.byref(nb)) == _lib.KC_ERR_INVALID_ARG
    assert pkg.lib().kc_dump_text_device(None, 0, 10, None, 0, None) == _lib.KC_ERR_INVALID_ARG
