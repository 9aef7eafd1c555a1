"""The kernels of kc_ctg_dedup in the shipped library (csrc/kc_dedup.hpp): compiled for gfx950, no scratch, no spills, and the
register counts DESIGN.md section 29 records.

The anchor, link and windows kernels are templated over the key's words, the windows kernel over its pass as well, the
verify kernel over the segmented path and the gather over the element size.  The windows kernel holds a key and its reverse
complement in two arrays of NL words, the verify kernel sixteen bytes of either side in four words each across the reversal,
the gather a chunk in four words across an unrolled loop: an index or a structure the compiler could not keep in registers
would show as scratch here.  The check of the block and the scans are kc_align.hpp's, kc_links.hpp's and kc_scan.hpp's own
kernels, of which the call adds no instantiation (tests/test_links_resources.py, tests/test_trim_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel and its template arguments as the mangled name spells them: VGPRs
WANT = {"kc_dedup_anchor_kernelILi1E": 13, "kc_dedup_anchor_kernelILi2E": 20, "kc_dedup_anchor_kernelILi3E": 25, "kc_dedup_anchor_kernelILi4E": 31,
        "kc_dedup_link_kernelILi1E": 16, "kc_dedup_link_kernelILi2E": 20, "kc_dedup_link_kernelILi3E": 26, "kc_dedup_link_kernelILi4E": 30,
        "kc_dedup_windows_kernelILi1ELb0E": 27, "kc_dedup_windows_kernelILi1ELb1E": 28, "kc_dedup_windows_kernelILi2ELb0E": 36,
        "kc_dedup_windows_kernelILi2ELb1E": 28, "kc_dedup_windows_kernelILi3ELb0E": 42, "kc_dedup_windows_kernelILi3ELb1E": 36,
        "kc_dedup_windows_kernelILi4ELb0E": 52, "kc_dedup_windows_kernelILi4ELb1E": 46,
        "kc_dedup_verify_kernelILb0E": 44, "kc_dedup_verify_kernelILb1E": 31, "kc_dedup_best_kernelE": 10, "kc_dedup_pick_kernelE": 14,
        "kc_dedup_status_kernelE": 22, "kc_dedup_records_kernelE": 20, "kc_dedup_gather_kernelILi1E": 31, "kc_dedup_gather_kernelILi2E": 31}


@needs_llvm
def test_dedup_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_dedup_" in n)
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
        assert not [t for t in TAKEN + ("kc_scaf_", "kc_close_", "kc_shuf_", "kc_asm_", "kc_fa_", "kc_rtext_") if t in n], n
