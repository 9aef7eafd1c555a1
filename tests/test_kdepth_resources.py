"""The kernels of kc_seq_kmer_depths and kc_count_spectrum in the shipped library (csrc/kc_kdepth.hpp): compiled for gfx950,
exactly the expected set, no scratch, no spills, and the register counts DESIGN.md section 31 records.

kc_ktrack_windows_kernel is templated on the words of a k-mer (1 to 4) and on KC_KDEPTH_FILL_MEAN; a lane holds the forward
and the reverse-complement words and, for the four windows whose probes are in flight together, their canonical keys and
slots: 8 x NL + 8 registers that the width adds, which is what separates the instantiations.  The widest stays under the 128
registers at which a workgroup of four waves still shares a SIMD with three others.  The calls launch no shared kernel, so
none gains an instance: the counts the other resource tests rely on are held here as they are."""
import re

from test_align_resources import WANT as ALIGN_WANT
from test_fastq_out_resources import COUNTS
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel: VGPRs; the windows kernel by (NL, FILL)
WANT = {"kc_ktrack_offsets_kernel": 12, "kc_ktrack_records_kernel": 28, "kc_ktrack_fill_kernel": 42, "kc_spect_hist_kernel": 17,
        "kc_spect_stats_kernel": 99}
WINDOWS = {(1, 0): 58, (1, 1): 56, (2, 0): 76, (2, 1): 73, (3, 0): 92, (3, 1): 89, (4, 0): 108, (4, 1): 107}
OTHERS = TAKEN + ("kc_scaf_", "kc_close_", "kc_shuf_", "kc_asm_", "kc_fq_", "kc_fa_", "kc_rtext_", "kc_dedup_", "kc_dump_")


@needs_llvm
def test_kdepth_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_ktrack_" in n or "kc_spect_" in n)
    assert len(names) == len(WANT) + len(WINDOWS), names
    for want, vgprs in WANT.items():
        mine = [n for n in names if want in n]
        assert len(mine) == 1, (want, names)
        assert md[mine[0]]["vgpr_count"] == vgprs, (want, md[mine[0]])
    seen = {}
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 128, (n, md[n])
        assert not [t for t in OTHERS if t in n], n
        m = re.search(r"kc_ktrack_windows_kernelILi(\d)ELb(\d)EE", n)
        if m:
            seen[(int(m.group(1)), int(m.group(2)))] = md[n]["vgpr_count"]
    assert seen == WINDOWS


@needs_llvm
def test_the_shared_kernels_gain_no_instance():
    md = kernel_metadata()
    for part, count in COUNTS.items():
        assert len([n for n in md if part in n]) == count, part
    assert len([n for n in md if "kc_align_" in n]) == sum(ALIGN_WANT.values())
