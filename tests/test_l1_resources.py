"""Registers of level 1's instantiations over six-byte records, read from the code object inside the shipped library:
kc_l1_reads16_kernel for the four input formats (ASCII reads, the case-masked block, read-cache bytes, reads with byte-loaded
qualities), with and without the shard filter, with k = 21 as a constant and k in registers; kc_l1_wire6_kernel and
kc_l1_records16_kernel, which share its scan, reserve and copy-out.  The bounds are the counts of the build before the
staging and the copy-out were slimmed (the benchmark's <0, false, 21>: 109): neither may cost a register, and nothing may
live in scratch -- a reload from scratch is a vector-memory load, and its wait is a wait for every prefetch load and copy-out
store the wave has in flight.  (kc_l1_records16_kernel had three registers in scratch, in its prologue, before; it may keep
them.)"""
import pytest

from test_kernel_resources import kernel_metadata, needs_llvm

# (FMT, shard filter, k) -> vector registers before
READS16 = {
    (0, 0, 21): 109, (0, 1, 21): 116, (0, 0, 0): 110, (0, 1, 0): 113,
    (1, 0, 21): 107, (1, 1, 21): 115, (1, 0, 0): 109, (1, 1, 0): 112,
    (2, 0, 21): 105, (2, 1, 21): 112, (2, 0, 0): 106, (2, 1, 0): 109,
    (3, 0, 21): 109, (3, 1, 21): 116, (3, 0, 0): 110, (3, 1, 0): 113,
}


@pytest.fixture(scope="module")
def md():
    return kernel_metadata()


def one(md, prefix):
    hits = [v for n, v in md.items() if n.startswith(prefix)]
    assert len(hits) == 1, prefix
    return hits[0]


@needs_llvm
@pytest.mark.parametrize("fmt,sh,kk", sorted(READS16))
def test_level_1_from_reads_costs_no_more_registers_than_before(md, fmt, sh, kk):
    k = one(md, "_ZN2kc20kc_l1_reads16_kernelILi%dELb%dELi%dEE" % (fmt, sh, kk))
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= READS16[(fmt, sh, kk)], k


@needs_llvm
def test_level_1_from_records_costs_no_more_registers_than_before(md):
    w6 = one(md, "_ZN2kc18kc_l1_wire6_kernelE")
    assert w6["vgpr_spill_count"] == 0 and w6["private_segment_fixed_size"] == 0 and w6["vgpr_count"] <= 115, w6
    r16 = one(md, "_ZN2kc22kc_l1_records16_kernelE")
    assert r16["vgpr_spill_count"] <= 3 and r16["private_segment_fixed_size"] <= 12 and r16["vgpr_count"] <= 128, r16
