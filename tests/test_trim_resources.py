"""The adapter-trim kernels of the shipped library (csrc/kc_trim.hpp): compiled for gfx950, no scratch, no spills.

As built (hipcc -O3, gfx950; VGPRs from the code object's notes, LDS from the declarations):
  kc_trim_seed_kernel    no LDS; one load of the bases, three shuffles and one table probe a round
  kc_trim_align_kernel   8 KiB LDS (the set of entries already aligned), one wave a workgroup; the alignment with 16 rows
                         a lane (adapters of 129..1024 bases) keeps H, E, the query codes and the two column temporaries
                         in registers
  kc_trim_sizes_kernel   32 B LDS
  kc_trim_write_kernel   3 KiB + 32 B LDS (in-tile offsets and lengths)
Registers as built: seed 41 VGPRs, align 225 VGPRs (both alignment widths and both passes are inlined into it; scalar
registers overflow into VGPR lanes there, not into memory), sizes and write below 32.
The bounds are what the design needs: the seed pass, which sees every read, at 64 VGPRs or fewer keeps eight waves a
SIMD; the align kernel runs one wave a workgroup on the few listed reads and only has to stay out of scratch."""
from test_kernel_resources import kernel_metadata, needs_llvm


@needs_llvm
def test_trim_kernels_do_not_spill():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_trim_" in n)
    assert len(names) == 4, names
    for want in ("kc_trim_seed_kernel", "kc_trim_align_kernel", "kc_trim_sizes_kernel", "kc_trim_write_kernel"):
        assert sum(1 for n in names if want in n) == 1, (want, names)
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= (256 if "align" in n else 64), (n, md[n])


@needs_llvm
def test_shared_scan_kernel_has_two_instances_without_scratch():
    """csrc/kc_scan.hpp: one array (FASTQ, trim) and two arrays (merge); the arrays' pointers are indexed at compile time,
    so neither instance keeps anything in private memory."""
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_scan_kernel" in n)
    assert len(names) == 2, names
    for n in names:
        print(n, md[n])
        assert md[n]["vgpr_spill_count"] == 0, n
        assert md[n]["private_segment_fixed_size"] == 0, n
