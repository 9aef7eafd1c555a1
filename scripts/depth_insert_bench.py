"""Times kc_aln_depths and kc_pair_inserts behind kc_align_reads and kc_align_gapped: paired reads of 150 bases cut from
random contigs of unitig-like lengths (scripts/gap_align_bench.py's contigs) with fragment lengths drawn from a normal
distribution, substitutions planted at an error rate, aligned and refined on the device.  Prints one JSON line and
writes it to profiles/aln_depths_<date>.json.

Reported: records/s of either call by kernel time (HIP events, KC_FLAG_TIME_KERNELS), every new kernel's launches and
time, and beside each pass the time a measured device-to-device copy takes for the bytes that pass must move (a copy of
n bytes moves 2n: the pass's reads and writes together are held against a copy of half their sum).  The histogram's mean
and deviation are printed beside the drawn ones.  No rate is fixed in advance.
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
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_input(rng, n_pairs, read_len, n_ctgs, error_rate, frag_mean, frag_sd):
    """(block, block offsets, bases, read offsets, drawn fragment lengths)"""
    lens = np.clip(rng.lognormal(7.0, 1.0, n_ctgs).astype(np.int64), read_len + 8, 100000)
    offs = np.zeros(n_ctgs + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens + 1)
    block = ACGT[rng.integers(0, 4, int(offs[-1]))]
    block[offs[1:].astype(np.int64) - 1] = ord("_")
    ctg = rng.integers(0, n_ctgs, n_pairs)
    f = np.clip(rng.normal(frag_mean, frag_sd, n_pairs).round().astype(np.int64), read_len, lens[ctg])  # a fragment lies inside its contig
    start = (rng.random(n_pairs) * (lens[ctg] - f + 1)).astype(np.int64) + offs[ctg].astype(np.int64)
    col = np.arange(read_len)
    m1 = block[start[:, None] + col]
    m2 = COMP[block[(start + f - 1)[:, None] - col]]  # the reverse complement of the fragment's last read_len bases
    reads = np.empty((2 * n_pairs, read_len), dtype=np.uint8)
    swap = rng.random(n_pairs) < 0.5
    reads[0::2] = np.where(swap[:, None], m2, m1)
    reads[1::2] = np.where(swap[:, None], m1, m2)
    err = rng.random(reads.shape) < error_rate
    reads[err] = ACGT[(np.searchsorted(ACGT, reads[err]) + 1 + rng.integers(0, 3, int(err.sum()))) % 4]
    roffs = np.arange(2 * n_pairs + 1, dtype=np.uint64) * np.uint64(read_len)
    return block, offs, reads.reshape(-1), roffs, f


def copy_ms(nbytes_moved, dev, reps=5):
    """median time of a device-to-device copy that moves this many bytes (reads and writes together)"""
    n = max(int(nbytes_moved) // 2, 1)
    src, dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    dst.copy_(src)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=400_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=20000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--frag-mean", type=float, default=400.0)
    ap.add_argument("--frag-sd", type=float, default=50.0)
    ap.add_argument("--max-insert", type=int, default=2000)
    ap.add_argument("--edge-clip", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aln_depths_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    block, offs, bases, roffs, f = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    nreads = 2 * a.pairs
    out = dict(metric="aln_depths", k=a.k, pairs=a.pairs, read_len=a.read_len, contigs=a.contigs, block_bytes=int(len(block)), error_rate=a.error_rate,
               drawn_mean=round(float(f.mean()), 3), drawn_stddev=round(float(f.std()), 3), max_insert=a.max_insert, edge_clip=a.edge_clip,
               host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, g_st = kc.align_gapped(d_bases, d_offs, alns)
        n = gaps.numel() // 32
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            _, _, d_st = kc.aln_depths(gaps, edge_clip=a.edge_clip, best_only=True, per_contig=True, nreads=nreads)
            kt_d = kc.kernel_times(clear=True)
            _, _, p_st = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
            kt_p = kc.kernel_times(clear=True)
            if r:
                runs.append((sum(v[1] for v in kt_d.values()) + sum(v[1] for v in kt_p.values()), kt_d, kt_p, d_st, p_st))
        runs.sort(key=lambda x: x[0])
        _, kt_d, kt_p, d_st, p_st = runs[len(runs) // 2]
        nb, nc = kc.contig_index_info()
        tiles = (nb + 2047) // 2048
        # bytes a pass must move: the records are 32 bytes, a difference 4, a depth 2, a best word 8, the contigs' partial figures 24
        must = {"kc_depth_check_kernel": 32 * n, "kc_depth_best_kernel": 32 * n + 8 * nreads, "kc_depth_mark_kernel": 32 * n + 8 * n + 8 * d_st["used"],
                "kc_depth_tile_sums_kernel": 4 * nb + 8 * tiles, "kc_depth_scan_kernel": 16 * tiles, "kc_depth_rescan_kernel": 4 * nb + 8 * tiles + 24 * nc,
                "kc_depth_ctg_kernel": (24 + 8 + 4 + 32) * nc, "kc_depth_fill_kernel": 2 * nb + 8 * nc,
                "kc_align_lengths_kernel<pair>": 8 * nreads, "kc_depth_check_kernel<pair>": 32 * n + 16 * n, "kc_depth_best_kernel<pair>": 32 * n + 8 * nreads,
                "kc_pair_classify_kernel": (16 + 64 + 16 + 16) * a.pairs, "kc_pair_classify_kernel<lds>": (16 + 64 + 16 + 16) * a.pairs}
        kernels = {}
        for name, v in list(kt_d.items()) + list(kt_p.items()):
            kernels[name] = dict(launches=v[0], total_ms=round(v[1], 4), bytes_moved=int(must.get(name, 0)),
                                 copy_of_those_bytes_ms=round(copy_ms(must[name], dev), 4) if name in must else None)
        d_ms, p_ms = sum(v[1] for v in kt_d.values()), sum(v[1] for v in kt_p.values())
        out.update(records=n, gap_stats=g_st, depth_stats=d_st, insert_stats=p_st, depth_kernel_ms=round(d_ms, 3), pair_kernel_ms=round(p_ms, 3),
                   runs_kernel_ms=[round(x[0], 3) for x in runs], depth_records_per_s=round(n / (d_ms / 1e3)) if d_ms else None,
                   pair_records_per_s=round(n / (p_ms / 1e3)) if p_ms else None, kernels=kernels)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
