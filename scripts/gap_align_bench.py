"""Times kc_align_gapped behind kc_align_reads: reads of 150 bases with a planted error rate (substitutions, and one error
in five an insertion or deletion of 1 to 3 bases) over random contigs of unitig-like lengths, indexed on the device.
Prints one JSON line and writes it to profiles/gap_align_<date>.json.

Reported: records/s and cell updates/s of kc_align_gapped by kernel time (HIP events, KC_FLAG_TIME_KERNELS; a cell is
one row of one column of one pass's window, counted once per record as kc_gap_stats.cells does, although the second
pass walks part of them again), every kc_gap_* kernel's time, the share of exact records, and beside that the kernel
time of kc_align_reads on the same reads -- the cost of the step this one follows.  No rate is fixed in advance.
--runs timed repetitions after one warm-up; the median by total kernel time is reported."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def make_input(rng, n_reads, read_len, n_ctgs, error_rate):
    """(block, block offsets, bases, read offsets, reads with an error, reads with an indel)"""
    lens = np.clip(rng.lognormal(7.0, 1.0, n_ctgs).astype(np.int64), read_len + 8, 100000)
    offs = np.zeros(n_ctgs + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens + 1)
    block = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offs[-1]))]
    block[offs[1:].astype(np.int64) - 1] = ord("_")
    ctg = rng.integers(0, n_ctgs, n_reads)
    start = (rng.random(n_reads) * (lens[ctg] - read_len - 4)).astype(np.int64) + offs[ctg].astype(np.int64)
    nerr = rng.binomial(read_len, error_rate, n_reads)
    flip = rng.random(n_reads) < 0.5
    reads, with_err, with_indel = [], 0, 0
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(n_reads):
        r = block[start[i]:start[i] + read_len + 4].copy()
        indel = False
        for _ in range(nerr[i]):
            if len(r) == 0:
                break
            p = int(rng.integers(0, min(read_len, len(r))))  # deletions shorten r
            kind = int(rng.integers(0, 10))
            if kind < 8:
                r[p] = acgt[(int(np.searchsorted(acgt, r[p])) + 1 + int(rng.integers(0, 3))) % 4]
            elif kind == 8:
                r = np.concatenate([r[:p], acgt[rng.integers(0, 4, int(rng.integers(1, 4)))], r[p:]])
                indel = True
            else:
                r = np.concatenate([r[:p], r[p + int(rng.integers(1, 4)):]])
                indel = True
        r = r[:read_len]
        if len(r) < read_len:
            r = np.concatenate([r, acgt[rng.integers(0, 4, read_len - len(r))]])
        reads.append(COMP[r[::-1]] if flip[i] else r)
        with_err += 1 if nerr[i] else 0
        with_indel += 1 if indel else 0
    bases = np.concatenate(reads)
    roffs = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)
    return block, offs, bases, roffs, with_err, with_indel


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=400_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=20000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gap_align_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    block, offs, bases, roffs, with_err, with_indel = make_input(rng, a.reads, a.read_len, a.contigs, a.error_rate)
    out = dict(metric="gap_align", k=a.k, reads=a.reads, read_len=a.read_len, contigs=a.contigs, contig_bases=int(len(block) - a.contigs),
               error_rate=a.error_rate, reads_with_an_error=with_err, reads_with_an_indel=with_indel, pad=a.pad, scores=list(pkg.kcount.BLASTN_ALN_SCORES),
               host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        out["index"] = kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            alns, _, a_st = kc.align_reads(d_bases, d_offs)
            kt_align = {n: v for n, v in kc.kernel_times(clear=True).items() if n.startswith("kc_align")}
            t0 = time.perf_counter()
            gap, g_st = kc.align_gapped(d_bases, d_offs, alns, pad=a.pad)
            wall = time.perf_counter() - t0
            kt_gap = {n: v for n, v in kc.kernel_times(clear=True).items() if n.startswith("kc_gap") or n.endswith("<gap>")}
            if r:
                runs.append((sum(v[1] for v in kt_gap.values()), kt_gap, kt_align, wall, a_st, g_st))
        runs.sort(key=lambda x: x[0])
        ms, kt_gap, kt_align, wall, a_st, g_st = runs[len(runs) // 2]
        align_ms = sum(v[1] for v in kt_align.values())
        out.update(align_stats=a_st, gap_stats=g_st, exact_share=round(g_st["exact"] / max(g_st["records"], 1), 4),
                   gap_kernel_ms=round(ms, 3), gap_wall_ms=round(wall * 1e3, 3), runs_gap_kernel_ms=[round(x[0], 3) for x in runs],
                   records_per_s=round(g_st["records"] / (ms / 1e3)) if ms else None,
                   cell_updates_per_s=round(g_st["cells"] / (kt_gap.get("kc_gap_dp_kernel", (0, 0))[1] / 1e3)) if kt_gap.get("kc_gap_dp_kernel", (0, 0))[1] else None,
                   gap_kernels={n: dict(launches=v[0], total_ms=round(v[1], 3)) for n, v in kt_gap.items()},
                   align_reads_kernel_ms=round(align_ms, 3),
                   align_reads_kernels={n: dict(launches=v[0], total_ms=round(v[1], 3)) for n, v in kt_align.items()})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
