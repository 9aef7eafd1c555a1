"""The scaffold kernels of the shipped library (csrc/kc_scaffold.hpp): compiled for gfx950, no scratch, no spills, and the
register counts DESIGN.md section 20 records.

None is templated.  The choose kernel carries a lane's best link and its second's support through six butterfly steps,
the writer a member's seven figures and sixteen bytes in four words across an unrolled loop, the weight kernel its two
nodes' weights in a two-element array: an index or a structure the compiler could not keep in registers would show as
scratch here.  The jump rounds, the cut and the scans are kc_unitig.hpp's and kc_scan.hpp's own kernels
(tests/test_unitig_resources.py, tests/test_trim_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm

# kernel: VGPRs
WANT = {"kc_scaf_check_kernel": 26, "kc_scaf_choose_kernel": 36, "kc_scaf_edge_kernel": 30, "kc_scaf_next_kernel": 12,
        "kc_scaf_weight_kernel": 26, "kc_scaf_select_kernel": 24, "kc_scaf_members_kernel": 16, "kc_scaf_records_kernel": 15,
        "kc_scaf_write_kernel": 36}
# substrings by which the other resource tests pick their kernels: no scaffold kernel's mangled name may hold one
TAKEN = ("kc_link_", "kc_unitig_", "kc_gap_", "kc_pair_", "kc_depth_", "kc_lassm_", "kc_align_", "kc_sort_", "kc_trim_", "kc_merge_",
         "kc_scan_kernel")


@needs_llvm
def test_scaffold_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_scaf_" in n)
    assert len(names) == len(WANT), names
    for want, vgprs in WANT.items():
        mine = [n for n in names if want in n]
        assert len(mine) == 1, (want, names)
        assert md[mine[0]]["vgpr_count"] == vgprs, (want, md[mine[0]])
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert not [t for t in TAKEN if t in n], n
