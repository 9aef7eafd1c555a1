"""The kernels of kc_ctg_polish in the shipped library (csrc/kc_polish.hpp): compiled for gfx950, exactly the expected set, no
scratch, no spills, and the register counts DESIGN.md section 33 records.

kc_polish_tile_kernel is templated on the pass (count, write); its loops over a lane's sixteen bytes are rolled over two 64-bit
halves, which is what keeps it under 64 registers (eight waves a SIMD beside 16 KiB of LDS a workgroup).  The call launches
kc_align_lengths_kernel, kc_depth_check_kernel, kc_depth_best_kernel, kc_sort_hist_kernel<false>, kc_sort_scatter_kernel,
kc_link_tile_scan_kernel and kc_scan_kernel<1> as they stand, so none gains an instance: the counts the other resource tests
rely on are held here as they are."""
import re

from test_correct_resources import EVAL as CORRECT_EVAL, SITES as CORRECT_SITES, WANT as CORRECT_WANT
from test_fastq_out_resources import COUNTS
from test_kdepth_resources import OTHERS, WANT as KDEPTH_WANT, WINDOWS as KDEPTH_WINDOWS
from test_kernel_resources import kernel_metadata, needs_llvm

# kernel: VGPRs; the tile kernel by pass
WANT = {"kc_polish_place_kernel": 42}
TILE = {0: 44, 1: 54}
# instances of kernels the call shares with other entry points
SHARED = {"kc_sort_hist_kernel": 2, "kc_sort_scatter_kernel": 1, "kc_depth_check_kernel": 1, "kc_depth_best_kernel": 1, "kc_align_lengths_kernel": 1}


@needs_llvm
def test_polish_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_polish_" in n)
    assert len(names) == len(WANT) + len(TILE), names
    for want, vgprs in WANT.items():
        mine = [n for n in names if want in n]
        assert len(mine) == 1, (want, names)
        assert md[mine[0]]["vgpr_count"] == vgprs, (want, md[mine[0]])
    tiles = {}
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 64, (n, md[n])  # eight waves a SIMD
        assert not [t for t in OTHERS + ("kc_ktrack_", "kc_spect_", "kc_correct_") if t in n], n
        m = re.search(r"kc_polish_tile_kernelILi(\d)EE", n)
        if m:
            tiles[int(m.group(1))] = md[n]["vgpr_count"]
    assert tiles == TILE


@needs_llvm
def test_the_shared_kernels_gain_no_instance():
    md = kernel_metadata()
    for part, count in list(COUNTS.items()) + list(SHARED.items()):
        assert len([n for n in md if part in n]) == count, part
    assert len([n for n in md if "kc_ktrack_" in n or "kc_spect_" in n]) == len(KDEPTH_WANT) + len(KDEPTH_WINDOWS)
    assert len([n for n in md if "kc_correct_" in n]) == len(CORRECT_WANT) + len(CORRECT_EVAL) + len(CORRECT_SITES)
