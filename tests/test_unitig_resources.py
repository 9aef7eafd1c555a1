"""The unitig kernels of the shipped library (csrc/kc_unitig.hpp): compiled for gfx950, no scratch, no spills, and at
most 64 VGPRs where a k-mer has up to three words (k <= 95), so that occupancy is never what limits the pointer jumping.

The links kernel is the only one templated on the words of a k-mer (one instantiation each for 1, 2, 3 and 4 words);
the other six take the width at run time or do not look at keys at all.

As built (hipcc -O3, gfx950), no LDS anywhere:
  kc_unitig_links_kernel<1..4>   24 / 28 / 36 / 46 VGPRs
  kc_unitig_min_jump_kernel      8      kc_unitig_rank_jump_kernel   6
  kc_unitig_cut_kernel           12     kc_unitig_select_kernel      16
  kc_unitig_write_kernel         17     kc_unitig_depth_kernel       24"""
import re

from test_kernel_resources import kernel_metadata, needs_llvm

WANT = {"kc_unitig_links_kernel": 4, "kc_unitig_min_jump_kernel": 1, "kc_unitig_cut_kernel": 1, "kc_unitig_rank_jump_kernel": 1,
        "kc_unitig_select_kernel": 1, "kc_unitig_write_kernel": 1, "kc_unitig_depth_kernel": 1}


@needs_llvm
def test_unitig_kernels_do_not_spill():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_unitig_" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert sum(1 for n in names if want in n) == count, (want, names)
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        m = re.search(r"kc_unitig_links_kernelILi(\d)E", n)
        if m is None or int(m.group(1)) <= 3:
            assert md[n]["vgpr_count"] <= 64, (n, md[n])
