"""The depth and insert-size kernels of the shipped library (csrc/kc_depth.hpp): compiled for gfx950, no scratch, no
spills, at most 128 registers.

kc_pair_classify_kernel is templated on where its histogram lives (LDS bins or global atomics); the others are not
templated.  The rescan holds a thread's eight depths, two open segments and the scan's temporaries in registers; an
index into those eight that the compiler could not resolve would show as scratch here."""
from test_kernel_resources import kernel_metadata, needs_llvm

WANT = {"kc_depth_check_kernel": 1, "kc_depth_best_kernel": 1, "kc_depth_mark_kernel": 1, "kc_depth_tile_sums_kernel": 1,
        "kc_depth_rescan_kernel": 1, "kc_depth_ctg_kernel": 1, "kc_depth_fill_kernel": 1, "kc_pair_classify_kernel": 2}


@needs_llvm
def test_depth_and_pair_kernels_do_not_spill():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_depth_" in n or "kc_pair_" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert sum(1 for n in names if want in n) == count, (want, names)
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 128, (n, md[n])
    assert {n for n in names if "kc_pair_classify_kernelILb" in n} == {n for n in names if "kc_pair_" in n}
