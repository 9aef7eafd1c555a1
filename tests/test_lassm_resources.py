"""The local-assembly kernels of the shipped library (csrc/kc_lassm.hpp): compiled for gfx950, no scratch, no spills, at most
128 registers.

kc_lassm_cands_kernel is templated on its pass (count or write); the others are not templated.  The walk kernel holds an
end's whole state in registers across its iterations and the write kernel sixteen bytes of the block; an index into
those that the compiler could not resolve would show as scratch here."""
from test_kernel_resources import kernel_metadata, needs_llvm

WANT = {"kc_lassm_pair_check_kernel": 1, "kc_lassm_cands_kernel": 2, "kc_lassm_plan_kernel": 1, "kc_lassm_text_kernel": 1,
        "kc_lassm_walk_kernel": 1, "kc_lassm_lens_kernel": 1, "kc_lassm_ends_kernel": 1, "kc_lassm_write_kernel": 1}


@needs_llvm
def test_local_assembly_kernels_do_not_spill():
    md = kernel_metadata()
    names = sorted(n for n in md if "kc_lassm_" in n)
    assert len(names) == sum(WANT.values()), names
    for want, count in WANT.items():
        assert sum(1 for n in names if want in n) == count, (want, names)
    for n in names:
        print(n, md[n])
        assert md[n].get("vgpr_spill_count", 0) == 0, n
        assert md[n].get("sgpr_spill_count", 0) == 0, n
        assert md[n].get("private_segment_fixed_size", 0) == 0, n
        assert md[n]["vgpr_count"] <= 128, (n, md[n])
    assert {n for n in names if "kc_lassm_cands_kernelILb" in n} == {n for n in names if "kc_lassm_cands_" in n}
