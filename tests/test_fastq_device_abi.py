"""kc_fastq_to_packed_device / kc_fastq_pairs_device without a GPU: the symbols are exported, a NULL context is refused,
and the kc_fq* kernels of the shipped library keep their registers."""
import ctypes as C

import pytest

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib
from test_kernel_resources import kernel_metadata, needs_llvm

TEXT = b"@r\nACGT\n+\nIIII\n"


def test_device_parsers_are_exported():
    so = C.CDLL(pkg.lib_path())
    for name in ("kc_fastq_to_packed_device", "kc_fastq_pairs_device"):
        assert hasattr(so, name), name
        assert name in _lib.SYMBOLS


def test_null_context_is_invalid_arg():
    L = pkg.lib()
    n, nb, c1, c2 = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    assert L.kc_fastq_to_packed_device(None, TEXT, len(TEXT), 0, 0, None, 0, None, 0, C.byref(n), C.byref(nb),
                                       C.byref(c1)) == _lib.KC_ERR_INVALID_ARG
    assert L.kc_fastq_pairs_device(None, TEXT, len(TEXT), TEXT, len(TEXT), 0, _lib.KC_FASTQ_PARTIAL, None, None, 0, None, 0,
                                   C.byref(n), C.byref(nb), C.byref(c1), C.byref(c2)) == _lib.KC_ERR_INVALID_ARG
    assert (n.value, nb.value) == (7, 7)


@needs_llvm
def test_fastq_kernels_do_not_spill():
    md = kernel_metadata()
    names = [n for n in md if "kc_fq_" in n]
    kinds = ("kc_fq_count", "kc_fq_index", "kc_fq_check", "kc_fq_detail", "kc_fq_sums", "kc_fq_write")
    for k in kinds:
        assert any(k in n for n in names), (k, names)
    assert len(names) == 7, names  # the write kernel twice: <packed> and <pairs>
    # the scan is the front end's shared kernel (csrc/kc_scan.hpp): the parser uses the one-array instance
    scans = [n for n in md if "kc_scan_kernelILi1E" in n]
    assert len(scans) == 1, scans
    for n in names + scans:
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
