"""The pair-merge kernels of the shipped library keep their registers: no vector register spills to scratch."""
import pytest

from test_kernel_resources import kernel_metadata, needs_llvm


@needs_llvm
def test_merge_kernels_do_not_spill():
    md = kernel_metadata()
    # the merge's scan is the two-array instance of the front end's shared kernel (csrc/kc_scan.hpp)
    names = [n for n in md if "kc_merge_decide" in n or "kc_merge_write" in n or "kc_scan_kernelILi2E" in n]
    assert len(names) == 5, names
    for n in names:
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
