"""The sort and dump-text kernels of the shipped library (csrc/kc_sort.hpp): compiled for gfx950, no scratch, no spills.

As built (hipcc -O3, gfx950):
  kc_sort_hist_kernel<load>, <carried>   1 KiB LDS (the digit histogram), about 10 VGPRs
  kc_sort_scatter_kernel                 62 KiB LDS (the tile's keys and indices in digit order, the ranks as u16, the
                                         4 x 256 counters), 86 VGPRs: the sixteen keys of a thread stay in registers
                                         (every index into them is a compile-time constant), the ranks are in LDS
  kc_sort_gather_kernel                  no LDS
  kc_dump_sizes_kernel                   16 B LDS
  kc_dump_write_kernel                   34 KiB LDS (256 lines of up to 136 bytes and the alignment shift)
The scatter's bound is what its LDS leaves room for anyway: two workgroups a CU, so 128 VGPRs cost no occupancy."""
from test_kernel_resources import kernel_metadata, needs_llvm

WANT = {"kc_sort_hist_kernel": 2, "kc_sort_scatter_kernel": 1, "kc_sort_gather_kernel": 1, "kc_dump_sizes_kernel": 1,
        "kc_dump_write_kernel": 1}


@needs_llvm
def test_sort_and_dump_kernels_do_not_spill():
    md = kernel_metadata()
    # (kc_dump_kernel, the table dump of kc_kernels.hpp, is not one of them)
    names = sorted(n for n in md if "kc_sort_" in n or "kc_dump_sizes" in n or "kc_dump_write" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert sum(1 for n in names if want in n) == count, (want, names)
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= (128 if "scatter" in n else 64), (n, md[n])
