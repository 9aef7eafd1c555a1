"""Registers of every instantiation of level 2 over six-byte level-1 records (kc_l2_rec6_kernel), read from the code object
inside the shipped library: the benchmark's <false, false>, the shard flow's <true, false> and the instalments' <false, true>
(the host pipe and a buffer smaller than the input).  None may keep anything in scratch: the prefetched pairs of the next
half-round wait in registers, and a reload from scratch would be a vector-memory load whose wait is a wait for every prefetch
load and copy-out store the wave has in flight."""
import pytest

from test_kernel_resources import kernel_metadata, needs_llvm


@needs_llvm
@pytest.mark.parametrize("fl,inc", [(0, 0), (1, 0), (0, 1)], ids=["plain", "shard-flow", "instalments"])
def test_level_2_of_six_byte_records_keeps_everything_in_registers(fl, inc):
    name = "_ZN2kc17kc_l2_rec6_kernelILb%dELb%dEE" % (fl, inc)
    hits = [v for n, v in kernel_metadata().items() if n.startswith(name)]
    assert len(hits) == 1, name
    k = hits[0]
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 128, k
