"""kc_build_unitigs rejects a NULL context and NULL count pointers before it touches a device (no GPU needed)."""
import ctypes as C

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib


def test_build_unitigs_null_context():
    nu, nb, st = C.c_uint64(7), C.c_uint64(7), _lib.kc_unitig_stats()
    L = pkg.lib()
    assert L.kc_build_unitigs(None, None, 0, None, None, 0, None, C.byref(nu), C.byref(nb), C.byref(st)) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_build_unitigs(None, None, 0, None, None, 0, None, None, None, None) == _lib.KC_ERR_INVALID_ARG
    assert (nu.value, nb.value) == (7, 7)  # nothing is written through the pointers of a call without a context


def test_build_unitigs_null_count_pointers():
    # the pointer checks come before the context is looked at: a context that is no context is never dereferenced
    nu, nb = C.c_uint64(0), C.c_uint64(0)
    L = pkg.lib()
    assert L.kc_build_unitigs(None, None, 0, None, None, 0, None, None, C.byref(nb), None) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_build_unitigs(None, None, 0, None, None, 0, None, C.byref(nu), None, None) == _lib.KC_ERR_INVALID_ARG


def test_unitig_stats_layout():
    assert C.sizeof(_lib.kc_unitig_stats) == 48
    assert [n for n, _ in _lib.kc_unitig_stats._fields_] == ["kmers", "unitigs", "singletons", "circular", "bases", "longest"]
