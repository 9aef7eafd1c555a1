"""The kernels of kc_ctg_select and kc_fasta_text in the shipped library (csrc/kc_asm.hpp): compiled for gfx950, no scratch,
no spills, and the register counts DESIGN.md section 23 records.

None is templated.  The writer carries a chunk's sixteen bytes in four words across an unrolled loop beside a record's
seven figures and the id's digits in a 64-bit word, the composition kernel six counters a lane: an index or a structure
the compiler could not keep in registers would show as scratch here.  The radix passes, the check of the block and the scans
are kc_sort.hpp's, kc_align.hpp's, kc_links.hpp's and kc_scan.hpp's own kernels, of which the two calls add no
instantiation (tests/test_links_resources.py, tests/test_trim_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel: VGPRs
WANT = {"kc_asm_lens_kernel": 20, "kc_asm_compact_kernel": 10, "kc_asm_sorted_kernel": 7, "kc_asm_nx_kernel": 12, "kc_asm_spans_kernel": 14,
        "kc_asm_comp_kernel": 34, "kc_asm_text_check_kernel": 8, "kc_asm_sizes_kernel": 16, "kc_asm_starts_kernel": 8, "kc_asm_write_kernel": 40}


@needs_llvm
def test_asm_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_asm_" in n)
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
        assert not [t for t in TAKEN + ("kc_scaf_", "kc_close_", "kc_shuf_") if t in n], n
