"""The gap-closing kernels of the shipped library (csrc/kc_close.hpp): compiled for gfx950, no scratch, no spills, and the
register counts DESIGN.md section 21 records.

Only the candidate kernel is templated (its count and its write pass).  The writer carries a member's eight figures and
sixteen bytes in four words across an unrolled loop, the vote four counters a lane, the decide kernel a lane's best (votes,
gap) word through six butterfly steps: an index or a structure the compiler could not keep in registers would show as
scratch here.  The grouping of the records and the scans are kc_links.hpp's and kc_scan.hpp's own kernels
(tests/test_links_resources.py, tests/test_trim_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm
from test_scaffold_resources import TAKEN

# kernel: VGPRs
WANT = {"kc_close_check_scaf_kernel": 8, "kc_close_claim_kernel": 4, "kc_close_check_member_kernel": 12, "kc_close_ends_kernel": 10,
        "kc_close_cands_kernelILb0EEE": 30, "kc_close_cands_kernelILb1EEE": 34, "kc_close_decide_kernel": 30, "kc_close_place_kernel": 20,
        "kc_close_vote_kernel": 28, "kc_close_records_kernel": 14, "kc_close_write_kernel": 38}


@needs_llvm
def test_close_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_close_" in n)
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
        assert not [t for t in TAKEN + ("kc_scaf_",) if t in n], n
