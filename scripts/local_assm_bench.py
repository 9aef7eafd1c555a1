"""Times kc_local_assm behind the device's own steps: scripts/depth_insert_bench.py's paired reads and contigs, with every
contig shortened by 200 bases at each end (less where it is short) after the reads were cut, so that reads hang over the
ends and mates fall beyond them.  index -> align_reads -> align_gapped -> pair_inserts -> aln_depths -> local_assm, all on
device tensors.  Prints one JSON line and writes it to profiles/local_assm_<date>.json.

Reported: ends/s and extension bases/s by kernel time (HIP events, KC_FLAG_TIME_KERNELS), every kernel's launches and
time, and beside each pass the time a measured device-to-device copy takes for the bytes that pass must move (a copy of
n bytes moves 2n).  The walk's bytes are summed over the ends from their records: per iteration the table's slots are
cleared (40 bytes each), the text is read (10 bytes a position) and a counter is updated per window.  No rate is fixed in
advance: there is no other implementation to compare with.
--runs timed repetitions after one warm-up; the median by total kernel time is reported."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from depth_insert_bench import copy_ms, make_input  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shorten(block, offs, cut):
    """every contig without its first and last min(cut, (len - 50) / 2) bases: (block, offsets, bases removed)"""
    lens = np.diff(offs.astype(np.int64)) - 1
    c = np.minimum(cut, np.maximum(0, (lens - 50) // 2))
    keep = np.ones(len(block), dtype=bool)
    starts = offs[:-1].astype(np.int64)
    for side in (starts, starts + lens - c):
        idx = np.repeat(side, c) + (np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c))
        keep[idx] = False
    new_offs = np.zeros(len(offs), dtype=np.uint64)
    new_offs[1:] = np.cumsum(lens - 2 * c + 1)
    return block[keep], new_offs, int(2 * c.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=400_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=20000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--frag-mean", type=float, default=400.0)
    ap.add_argument("--frag-sd", type=float, default=50.0)
    ap.add_argument("--cut", type=int, default=200)
    ap.add_argument("--max-insert", type=int, default=1000)
    ap.add_argument("--max-walk-len", type=int, default=400)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_assm_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    block, offs, bases, roffs, f = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    block, offs, removed = shorten(block, offs, a.cut)
    nreads = 2 * a.pairs
    out = dict(metric="local_assm", k=a.k, pairs=a.pairs, read_len=a.read_len, contigs=a.contigs, block_bytes=int(len(block)), bases_removed=removed,
               error_rate=a.error_rate, max_insert=a.max_insert, max_walk_len=a.max_walk_len, host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, g_st = kc.align_gapped(d_bases, d_offs, alns)
        _, pairs, p_st = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
        _, ctgs, _ = kc.aln_depths(gaps)
        n = gaps.numel() // 32
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            seqs, new_offs, ends, st = kc.local_assm(d_bases, None, d_offs, gaps, pairs, ctgs, max_insert=a.max_insert, max_walk_len=a.max_walk_len)
            kt = kc.kernel_times(clear=True)
            if r:
                runs.append((sum(v[1] for v in kt.values()), kt, st))
        runs.sort(key=lambda x: x[0])
        total_ms, kt, st = runs[len(runs) // 2]
        e = ends.cpu().numpy().view(pkg.kcount.LASSM_END_DTYPE)
        n_ends, total = len(e), int(seqs.numel())
        walked = e[e["status"] >= 2]
        cand_bases = walked["cands"].astype(np.int64) * a.read_len
        slots = 2 ** np.ceil(np.log2(np.maximum(2 * cand_bases, 2))).astype(np.int64)
        text = cand_bases + walked["cands"]
        walk_bytes = int((walked["iters"].astype(np.int64) * (2 * 40 * slots + 10 * text + 8 * cand_bases)).sum())
        n_cands, n_text = int(walked["cands"].sum()), int(text.sum())
        # bytes a pass must move: a record is 32 bytes, a pair 16, an offset 8, a candidate's entry 16, a text position 10
        must = {"kc_align_lengths_kernel<lassm>": 8 * nreads, "kc_depth_check_kernel<lassm>": 32 * n + 16 * n, "kc_lassm_pair_check_kernel": (16 + 64) * a.pairs,
                "kc_lassm_cands_kernel<count>": (8 + 16 + 64) * nreads + 16 * st["cands_overhang"] + 16 * st["cands_mate"],
                "kc_lassm_plan_kernel": (16 + 24 + 16) * n_ends, "kc_lassm_scan_kernel": 16 * (3 * n_ends + n_ends // 2),
                "kc_lassm_cands_kernel<write>": (8 + 16 + 64) * nreads + (16 + 8 + 16) * n_cands, "kc_lassm_text_kernel": 16 * n_cands + 2 * int(cand_bases.sum()) + 10 * n_text,
                "kc_lassm_walk_kernel": walk_bytes, "kc_lassm_lens_kernel": (32 + 8 + 8) * (n_ends // 2), "kc_lassm_ends_kernel": (16 + 8 + 8 + 16) * n_ends,
                "kc_lassm_write_kernel": 2 * total}
        kernels = {}
        for name, v in kt.items():
            kernels[name] = dict(launches=v[0], total_ms=round(v[1], 4), bytes_moved=int(must.get(name, 0)),
                                 copy_of_those_bytes_ms=round(copy_ms(must[name], dev), 4) if name in must else None)
        out.update(records=n, gap_stats=g_st, insert_stats=p_st, lassm_stats=st, new_block_bytes=total, kernel_ms=round(total_ms, 3),
                   runs_kernel_ms=[round(x[0], 3) for x in runs], ends_per_s=round(n_ends / (total_ms / 1e3)) if total_ms else None,
                   ext_bases_per_s=round(st["ext_bases"] / (total_ms / 1e3)) if total_ms else None, kernels=kernels)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
