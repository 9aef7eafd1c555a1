"""The kernels of kc_ctg_break in the shipped library (csrc/kc_break.hpp): compiled for gfx950, exactly the expected set, no
scratch and no spills.  The register counts are recorded in DESIGN.md section 34, not fixed here; eight waves a SIMD (64
registers or fewer) is what the test holds them to.

The call launches kc_align_lengths_kernel, kc_depth_check_kernel, kc_lassm_pair_check_kernel, kc_scan_kernel<1> and
kc_scan_kernel<2> as they stand, so none gains an instance: the counts the other resource tests rely on are held here as they are."""
import re

from test_fastq_out_resources import COUNTS
from test_kernel_resources import kernel_metadata, needs_llvm
from test_polish_resources import SHARED, TILE as POLISH_TILE, WANT as POLISH_WANT

# kernel -> instances
WANT = {"kc_break_mark_kernel": 1, "kc_break_tile_sums_kernel": 1, "kc_break_rescan_kernel": 1, "kc_break_tile_max_kernel": 1,
        "kc_break_runs_kernel": 2, "kc_break_records_kernel": 1, "kc_break_gather_kernel": 2, "kc_break_tracks_kernel": 1}


@needs_llvm
def test_break_kernels_do_not_spill_and_fit_eight_waves():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_break_" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert len([n for n in names if want in n]) == count, (want, names)
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 64, (n, md[n])
    assert sorted(int(m.group(1)) for m in (re.search(r"kc_break_runs_kernelILb(\d)EE", n) for n in names) if m) == [0, 1]
    assert sorted(int(m.group(1)) for m in (re.search(r"kc_break_gather_kernelILi(\d)EE", n) for n in names) if m) == [1, 2]


@needs_llvm
def test_the_shared_kernels_gain_no_instance():
    md = kernel_metadata()
    for part, count in list(COUNTS.items()) + list(SHARED.items()) + [("kc_lassm_pair_check_kernel", 1), ("kc_scan_kernelILi2E", 1)]:
        assert len([n for n in md if part in n]) == count, part
    assert len([n for n in md if "kc_polish_" in n]) == len(POLISH_WANT) + len(POLISH_TILE)
