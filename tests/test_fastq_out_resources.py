"""The kernels of kc_fastq_text in the shipped library (csrc/kc_fastq_out.hpp): compiled for gfx950, exactly the expected set,
no scratch, no spills, and the register counts DESIGN.md section 27 records.

None is templated.  The writer carries a chunk's sixteen bytes in four words across its loop over the chunk's records, beside a
record's seven figures, the six places at which its parts begin, sixteen loaded bytes and the number's digits in a 64-bit
word: an index or a structure the compiler could not keep in registers would show as scratch here.  The scans and the span table are
kc_links.hpp's, kc_scan.hpp's and kc_asm.hpp's own kernels, of which the call adds no instantiation
(tests/test_links_resources.py, tests/test_trim_resources.py, tests/test_asm_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel: VGPRs
WANT = {"kc_rtext_check_kernel": 8, "kc_rtext_bytes_kernel": 29, "kc_rtext_detail_kernel": 16, "kc_rtext_sizes_kernel": 12,
        "kc_rtext_starts_kernel": 8, "kc_rtext_write_kernel": 64}
# the counts the other resource tests rely on
COUNTS = {"kc_fq_": 7, "kc_asm_": 10, "kc_scan_kernelILi1E": 1, "kc_link_tile_scan_kernel": 1}


@needs_llvm
def test_fastq_out_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_rtext_" in n)
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
        assert not [t for t in TAKEN + ("kc_scaf_", "kc_close_", "kc_shuf_", "kc_asm_", "kc_fq_", "kc_fa_") if t in n], n
    for part, count in COUNTS.items():
        assert len([n for n in md if part in n]) == count, part
