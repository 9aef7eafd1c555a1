"""The read-shuffle kernels of the shipped library (csrc/kc_shuffle.hpp): compiled for gfx950, no scratch, no spills, and the
register counts DESIGN.md section 22 records.

None is templated.  The gather holds two aligned 16-byte source words, picks five of their eight dwords by the source's
misalignment and funnels them into four; the key kernel chooses between two loaded records: an index or a structure
the compiler could not keep in registers would show as scratch here.  The radix passes and the scans are kc_sort.hpp's,
kc_links.hpp's and kc_scan.hpp's own kernels (tests/test_sort_resources.py, tests/test_links_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel: VGPRs
WANT = {"kc_shuf_longest_kernel": 6, "kc_shuf_key_kernel": 14, "kc_shuf_place_kernel": 24, "kc_shuf_offsets_kernel": 14,
        "kc_shuf_gather_kernel": 33, "kc_shuf_remap_kernel": 14, "kc_shuf_parts_kernel": 14}


@needs_llvm
def test_shuffle_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_shuf_" in n)
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
        assert not [t for t in TAKEN + ("kc_scaf_", "kc_close_") if t in n], n
