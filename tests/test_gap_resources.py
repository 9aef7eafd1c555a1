"""The gapped-alignment kernels of the shipped library (csrc/kc_gap.hpp): compiled for gfx950, no scratch, no spills.

kc_gap_dp_kernel is templated on the rows a lane holds (1, 3, 8, 16: a 150-base read costs three); check and sort are
not templated.  A lane keeps H, E and the column's uncorrected H for each of its rows in registers, so the widest
instantiation must stay within the 128 registers at which a workgroup of four waves still shares a SIMD with others."""
import re

from test_kernel_resources import kernel_metadata, needs_llvm

WANT = {"kc_gap_check_kernel": 1, "kc_gap_sort_kernel": 1, "kc_gap_dp_kernel": 4}


@needs_llvm
def test_gap_kernels_do_not_spill():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_gap_" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert sum(1 for n in names if want in n) == count, (want, names)
    rows = set()
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 128, (n, md[n])
        m = re.search(r"kc_gap_dp_kernelILi(\d+)EE", n)
        if m:
            rows.add(int(m.group(1)))
    assert rows == {1, 3, 8, 16}
