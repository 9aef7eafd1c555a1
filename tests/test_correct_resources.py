"""The kernels of kc_correct_reads in the shipped library (csrc/kc_correct.hpp): compiled for gfx950, exactly the expected set,
no scratch, no spills, and the register counts DESIGN.md section 32 records.

kc_correct_eval_kernel is templated on the words of a k-mer (1 to 4): a lane holds one window's forward and reverse-complement
words and the canonical of the two, 3 x NL registers that the width adds.  kc_correct_sites_kernel is templated on the pass
(count, write); it keeps its eighteen positions as three bit masks, not as an array.  The call launches kc_ktrack_offsets_kernel,
kc_ktrack_windows_kernel<NL, false> and kc_scan_kernel<1> as they stand, so none gains an instance: the counts the other resource
tests rely on are held here as they are."""
import re

from test_fastq_out_resources import COUNTS
from test_kdepth_resources import OTHERS, WANT as KDEPTH_WANT, WINDOWS as KDEPTH_WINDOWS
from test_kernel_resources import kernel_metadata, needs_llvm

# kernel: VGPRs; the evaluation by NL, the sites by pass
WANT = {"kc_correct_apply_kernel": 16, "kc_correct_records_kernel": 13}
EVAL = {1: 26, 2: 32, 3: 36, 4: 42}
SITES = {0: 44, 1: 44}


@needs_llvm
def test_correct_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_correct_" in n)
    assert len(names) == len(WANT) + len(EVAL) + len(SITES), names
    for want, vgprs in WANT.items():
        mine = [n for n in names if want in n]
        assert len(mine) == 1, (want, names)
        assert md[mine[0]]["vgpr_count"] == vgprs, (want, md[mine[0]])
    evals, sites = {}, {}
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 64, (n, md[n])  # eight waves a SIMD
        assert not [t for t in OTHERS + ("kc_ktrack_", "kc_spect_") if t in n], n
        m = re.search(r"kc_correct_eval_kernelILi(\d)EE", n)
        if m:
            evals[int(m.group(1))] = md[n]["vgpr_count"]
        m = re.search(r"kc_correct_sites_kernelILb(\d)EE", n)
        if m:
            sites[int(m.group(1))] = md[n]["vgpr_count"]
    assert evals == EVAL and sites == SITES


@needs_llvm
def test_the_shared_kernels_gain_no_instance():
    md = kernel_metadata()
    for part, count in COUNTS.items():
        assert len([n for n in md if part in n]) == count, part
    assert len([n for n in md if "kc_ktrack_" in n or "kc_spect_" in n]) == len(KDEPTH_WANT) + len(KDEPTH_WINDOWS)
