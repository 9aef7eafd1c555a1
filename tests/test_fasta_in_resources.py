"""The kernels of kc_fasta_to_block in the shipped library (csrc/kc_fasta_in.hpp): compiled for gfx950, exactly the set
DESIGN.md section 24 lists, no scratch, no spills, and the register counts that section records.

None is templated.  The writer carries a chunk's sixteen bytes in four words and their depths in eight across an unrolled
loop beside a line's five figures, the check two counters, a key and a line's four figures: an index or a structure the
compiler could not keep in registers would show as scratch here.  The line index, the scans and the span search of the
writer are kc_fastq.hpp's, kc_scan.hpp's, kc_links.hpp's and kc_asm.hpp's own kernels and helpers, of which the call adds no
instantiation: the counts the other resource tests pin stay as they are."""
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel: VGPRs
WANT = {"kc_fa_lines_kernel": 12, "kc_fa_starts_kernel": 14, "kc_fa_spans_kernel": 16, "kc_fa_check_kernel": 32, "kc_fa_detail_kernel": 4,
        "kc_fa_recs_kernel": 28, "kc_fa_write_kernel": 54}


@needs_llvm
def test_fasta_in_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_fa_" in n)
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
        assert not [t for t in TAKEN + ("kc_scaf_", "kc_close_", "kc_shuf_", "kc_asm_", "kc_fq_") if t in n], n


@needs_llvm
def test_the_shared_kernels_gain_no_instance():
    md = kernel_metadata()
    assert len([n for n in md if "kc_fq_" in n]) == 7 and len([n for n in md if "kc_asm_" in n]) == 10
    assert len([n for n in md if "kc_scan_kernelILi1E" in n]) == 1 and len([n for n in md if "kc_link_tile_scan_kernel" in n]) == 1
