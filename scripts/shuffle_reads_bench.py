"""Times kc_shuffle_reads behind kc_align_reads, kc_align_gapped and kc_pair_inserts, and what the new order is worth to the
steps behind it: scripts/depth_insert_bench.py's input (paired reads of 150 bases cut from random contigs of unitig-like
lengths, every pair on a contig drawn at random, so the pairs come dealt in random order; fragment lengths from a normal
distribution, substitutions planted at an error rate), with qualities.  Prints one JSON line and writes it to
profiles/shuffle_reads_<date>.json.

Reported: every kernel's launches and time (HIP events, KC_FLAG_TIME_KERNELS); the gather's rate as bytes read plus
bytes written over its kernel time, beside the time and rate of a device-to-device copy that moves the same number of
bytes, made in the same run -- that copy is the yardstick, no figure chosen in advance; and the kernel time of
kc_align_reads and of kc_local_assm on the same reads before and after the shuffle (the records and pairs renumbered by
the call), each the median of --runs repetitions after a warm-up.  No threshold is set on the locality effect."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from depth_insert_bench import copy_ms, make_input  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(kc, runs, call):
    """(median total kernel ms, that run's {kernel: (launches, ms)}, the last result) of `call`, after one warm-up"""
    got, res = [], None
    for r in range(runs + 1):
        kc.kernel_times(clear=True)
        res = call()
        kt = kc.kernel_times(clear=True)
        if r:
            got.append((sum(v[1] for v in kt.values()), kt))
    got.sort(key=lambda x: x[0])
    return got[len(got) // 2][0], got[len(got) // 2][1], res, [round(x[0], 3) for x in got]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=400_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=40000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--frag-mean", type=float, default=400.0)
    ap.add_argument("--frag-sd", type=float, default=50.0)
    ap.add_argument("--max-insert", type=int, default=2000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle_reads_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    block, offs, bases, roffs, _ = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    quals = rng.integers(35, 74, size=len(bases)).astype(np.uint8)
    out = dict(metric="shuffle_reads", k=a.k, pairs=a.pairs, read_len=a.read_len, contigs=a.contigs, block_bytes=int(len(block)),
               error_rate=a.error_rate, parts=a.parts, host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_quals = torch.from_numpy(bases).to(dev), torch.from_numpy(quals).to(dev)
        d_offs = torch.from_numpy(roffs.view(np.int64)).to(dev)
        align_ms, _, (alns, _, _), align_runs = timed(kc, a.runs, lambda: kc.align_reads(d_bases, d_offs))
        gaps, _ = kc.align_gapped(d_bases, d_offs, alns)
        _, pairs, p_st = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
        lassm_kw = dict(max_insert=a.max_insert)
        lassm_ms, _, lassm, lassm_runs = timed(kc, a.runs, lambda: kc.local_assm(d_bases, d_quals, d_offs, gaps, pairs, **lassm_kw))
        ms, kt, s, runs = timed(kc, a.runs, lambda: kc.shuffle_reads(d_bases, d_quals, d_offs, gaps, pairs, parts=a.parts))
        st = s["stats"]
        moved = 4 * st["bytes"]  # bases and qualities, each read once and written once
        g_ms = kt["kc_shuf_gather_kernel"][1]
        c_ms = copy_ms(moved, dev)
        align2_ms, _, _, align2_runs = timed(kc, a.runs, lambda: kc.align_reads(s["bases"], s["offsets"]))
        lassm2_ms, _, lassm2, lassm2_runs = timed(kc, a.runs, lambda: kc.local_assm(s["bases"], s["quals"], s["offsets"], s["gap_alns"], s["pairs"],
                                                                                      **lassm_kw))
        same_assembly = bool(torch.equal(lassm[0], lassm2[0]) and torch.equal(lassm[1], lassm2[1]))
        out.update(records=gaps.numel() // 32, insert_classes=p_st["cls"], shuffle_stats=st, kernel_ms=round(ms, 3), runs_kernel_ms=runs,
                   pairs_per_s=round(a.pairs / (ms / 1e3)) if ms else None,
                   kernels={n: dict(launches=v[0], total_ms=round(v[1], 4)) for n, v in kt.items()},
                   gather=dict(bytes_moved=int(moved), ms=round(g_ms, 4), tb_per_s=round(moved / (g_ms / 1e3) / 1e12, 3) if g_ms else None,
                               copy_of_those_bytes_ms=round(c_ms, 4), copy_tb_per_s=round(moved / (c_ms / 1e3) / 1e12, 3) if c_ms else None,
                               share_of_copy_rate=round(c_ms / g_ms, 3) if g_ms else None),
                   align_reads_kernel_ms=dict(before=round(align_ms, 3), after=round(align2_ms, 3), runs_before=align_runs, runs_after=align2_runs),
                   local_assm_kernel_ms=dict(before=round(lassm_ms, 3), after=round(lassm2_ms, 3), runs_before=lassm_runs, runs_after=lassm2_runs,
                                             same_contigs_out=same_assembly))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
