"""The alignment kernels of the shipped library (csrc/kc_align.hpp): compiled for gfx950, no scratch, no spills.

kc_align_index_kernel is templated on the words of a k-mer (1 to 4), kc_align_reads_kernel on those and on the windows
a lane holds (1, 3, 8, 16: a 150-base read costs three); check, sweep and lengths look at no keys.  A lane of the reads
kernel keeps its candidates in registers -- two per window -- so the widest instantiation must stay under the 128
registers at which a workgroup of four waves still shares a SIMD with others."""
import re

from test_kernel_resources import kernel_metadata, needs_llvm

WANT = {"kc_align_check_kernel": 1, "kc_align_index_kernel": 4, "kc_align_sweep_kernel": 1, "kc_align_lengths_kernel": 1,
        "kc_align_reads_kernel": 16}


@needs_llvm
def test_align_kernels_do_not_spill():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_align_" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert sum(1 for n in names if want in n) == count, (want, names)
    combos = set()
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 128, (n, md[n])
        m = re.search(r"kc_align_reads_kernelILi(\d)ELi(\d+)EE", n)
        if m:
            combos.add((int(m.group(1)), int(m.group(2))))
    assert combos == {(nl, w) for nl in (1, 2, 3, 4) for w in (1, 3, 8, 16)}
