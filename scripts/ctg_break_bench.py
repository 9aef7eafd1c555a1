"""Times kc_ctg_break behind kc_align_reads, kc_align_gapped and kc_pair_inserts: scripts/depth_insert_bench.py's construction
(paired reads of 150 bases cut from random contigs, fragment lengths from a normal distribution, substitutions at an error
rate), with a share of the contigs joined pairwise into chimeras before they are indexed: the separator between contig 2i and
2i + 1 is left out, so no read pair spans the join.  Prints one JSON line and writes it to profiles/ctg_break_<date>.json.

Reported: kernel time per new kernel (HIP events, KC_FLAG_TIME_KERNELS), the whole call beside kc_aln_depths over the same
records in the same run, the gather beside a device-to-device copy of the same bytes in the same run, the planted joins cut (a
break within a read length of the join) and the true contigs cut wrongly (every other break).  No rate is fixed in advance.
--runs timed repetitions after one warm-up; the median by total kernel time is reported."""
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


def join_pairs(block, offs, share, min_len):
    """the block with the separator between contigs 2i and 2i + 1 left out for the first share of the pairs whose halves both
    have min_len bases: (block, offsets, block positions of the joins in the new block)"""
    n = len(offs) - 1
    lens = np.diff(offs.astype(np.int64)) - 1
    drop = np.zeros(n, dtype=bool)  # contig u's separator goes
    first = np.arange(0, int(n * share) // 2 * 2, 2)
    ok = (lens[first] >= min_len) & (lens[first + 1] >= min_len)
    drop[first[ok]] = True
    seps = offs[1:].astype(np.int64) - 1
    keep = np.ones(len(block), dtype=bool)
    keep[seps[drop]] = False
    new_block = block[keep]
    shift = np.cumsum(~keep)  # bytes removed up to and with each position
    joins = seps[drop] - (shift[seps[drop]] - 1)  # the first base behind the join, in the new block
    new_offs = np.concatenate(([0], (seps[~drop] - shift[seps[~drop]] + 1))).astype(np.uint64)
    return new_block, new_offs, joins


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=400_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=2000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--frag-mean", type=float, default=400.0)
    ap.add_argument("--frag-sd", type=float, default=50.0)
    ap.add_argument("--max-insert", type=int, default=800)
    ap.add_argument("--share", type=float, default=0.1, help="of the contigs that are joined pairwise")
    ap.add_argument("--max-span", type=int, default=-1, help="-1: a quarter of the mean physical coverage")
    ap.add_argument("--min-disc", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctg_break_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    true_block, true_offs, bases, roffs, f = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    block, offs, joins = join_pairs(true_block, true_offs, a.share, 2 * a.max_insert)
    coverage = float(f.sum()) / max(len(block) - (len(offs) - 1), 1)
    max_span = a.max_span if a.max_span >= 0 else int(coverage / 4)
    kw = dict(max_insert=a.max_insert, max_span=max_span, min_disc=a.min_disc, margin=a.max_insert, min_run=1)
    out = dict(metric="ctg_break", k=a.k, pairs=a.pairs, read_len=a.read_len, contigs=int(len(offs) - 1), joined=int(len(joins)), block_bytes=int(len(block)),
               error_rate=a.error_rate, physical_coverage=round(coverage, 2), params=kw, host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, _ = kc.align_gapped(d_bases, d_offs, alns)
        _, pairs, p_st = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
        depths, _, _ = kc.aln_depths(gaps)
        n = gaps.numel() // 32
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            kc.aln_depths(gaps)
            kt_d = kc.kernel_times(clear=True)
            res = kc.break_contigs(d_offs, gaps, pairs, depths=depths, tracks=True, **kw)
            kt_b = {k_: v for k_, v in kc.kernel_times(clear=True).items() if v[0]}
            if r:
                runs.append((sum(v[1] for v in kt_b.values()), kt_b, sum(v[1] for v in kt_d.values()), res))
        runs.sort(key=lambda x: x[0])
        b_ms, kt_b, d_ms, res = runs[len(runs) // 2]
        st, brk = res[5], res[4].cpu().numpy().view(pkg.BREAK_DTYPE)
        at = offs.astype(np.int64)[brk["ctg"]] + brk["pos"].astype(np.int64)  # block positions of the cuts
        near = np.abs(at[:, None] - joins[None, :]).min(axis=1) <= a.read_len if len(joins) and len(at) else np.zeros(len(at), dtype=bool)
        cut = int((np.abs(joins[:, None] - at[None, :]).min(axis=1) <= a.read_len).sum()) if len(joins) and len(at) else 0
        total = int(res[0].numel())
        slowest = max(kt_b.items(), key=lambda kv: kv[1][1])
        # the wrapper asks for the sizes first: what runs twice is halved for one call's worth
        one_call = sum(v[1] / (2 if v[0] == 2 and name not in ("kc_break_tracks_kernel",) else 1) for name, v in kt_b.items())
        out.update(records=n, insert_stats=p_st, break_stats=st, kernels={name: dict(launches=v[0], total_ms=round(v[1], 4)) for name, v in kt_b.items()},
                   wrapper_kernel_ms=round(b_ms, 3), one_call_kernel_ms=round(one_call, 3), aln_depths_kernel_ms=round(d_ms, 3),
                   runs_kernel_ms=[round(x[0], 3) for x in runs], slowest=slowest[0],
                   gather_ms=round(kt_b.get("kc_break_gather_kernel", (0, 0.0))[1], 4), copy_of_the_block_ms=round(copy_ms(2 * total, dev), 4),
                   planted_joins=int(len(joins)), planted_joins_cut=cut, true_contigs_cut_wrongly=int((~near).sum()))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
