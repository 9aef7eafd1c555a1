"""The contig-link kernels of the shipped library (csrc/kc_links.hpp): compiled for gfx950, no scratch, no spills, and the
register counts DESIGN.md section 19 records.

kc_link_group_kernel and kc_link_cands_kernel are templated on their pass (count or write); the others are not
templated.  The span branch of the candidate kernel holds two mates' distances and ends in two-element arrays and the
reduce kernel a run's seven figures across six shuffle steps; an index or a structure the compiler could not keep in
registers would show as scratch here.  The radix passes are kc_sort.hpp's own kernels (tests/test_sort_resources.py)."""
from test_kernel_resources import kernel_metadata, needs_llvm

# kernel: (instantiations, VGPRs of each in the order of their mangled names)
WANT = {"kc_link_group_kernel": (2, [12, 21]), "kc_link_cands_kernel": (2, [28, 36]), "kc_link_tile_scan_kernel": (1, [32]),
        "kc_link_heads_kernel": (1, [6]), "kc_link_reduce_kernel": (1, [39]), "kc_link_emit_kernel": (1, [18]),
        "kc_link_end_first_kernel": (1, [12])}


@needs_llvm
def test_link_kernels_do_not_spill_and_keep_their_registers():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_link_" in n)
    assert len(names) == sum(c for c, _ in WANT.values()), names
    for want, (count, vgprs) in WANT.items():
        mine = [n for n in names if want in n]
        assert len(mine) == count, (want, names)
        assert [md[n]["vgpr_count"] for n in mine] == vgprs, (want, [md[n] for n in mine])
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
    assert {n for n in names if "kernelILb" in n} == {n for n in names if "kc_link_group_" in n or "kc_link_cands_" in n}
