"""Times kc_ctg_polish behind kc_align_reads and kc_align_gapped on scripts/depth_insert_bench.py's input (paired reads of 150
bases cut from random contigs of unitig-like lengths, substitutions planted in the reads at an error rate), with substitutions
planted in the contigs as well: the index is built over the planted block, the reads come from the true one.  Prints one JSON
line and writes it to profiles/ctg_polish_<date>.json.

Reported: every kc_polish_* kind's launches and kernel time (HIP events, KC_FLAG_TIME_KERNELS; the median call of --runs after
a warm-up) without fixes (one tile pass) and with them (count and write pass), the votes per second of the tile kernel, and of
the planted errors how many the polished block holds restored, beside the bytes changed wrongly (different from the planted
block and from the true one).  The yardsticks come from the same run, no figure chosen in advance: kc_aln_depths' kernel time
over the same records, and a device-to-device copy of the block.  Needs a GPU: there is no fallback."""
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
from depth_insert_bench import ACGT, copy_ms, make_input  # noqa: E402
from shuffle_reads_bench import timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=400_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=40000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--contig-error-rate", type=float, default=0.002)
    ap.add_argument("--frag-mean", type=float, default=400.0)
    ap.add_argument("--frag-sd", type=float, default=50.0)
    ap.add_argument("--min-depth", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=700)
    ap.add_argument("--edge-clip", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctg_polish_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("polish_bench.py needs a GPU: the HIP path is the only path")
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    true_block, offs, bases, roffs, _ = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    planted = (rng.random(len(true_block)) < a.contig_error_rate) & (true_block != ord("_"))
    block = true_block.copy()
    block[planted] = ACGT[(np.searchsorted(ACGT, true_block[planted]) + 1 + rng.integers(0, 3, int(planted.sum()))) % 4]
    out = dict(metric="ctg_polish", k=a.k, pairs=a.pairs, read_len=a.read_len, contigs=a.contigs, block_bytes=int(len(block)),
               error_rate=a.error_rate, contig_error_rate=a.contig_error_rate, planted=int(planted.sum()), min_depth=a.min_depth,
               min_permille=a.min_permille, edge_clip=a.edge_clip, host_input_s=round(time.perf_counter() - t0, 1))
    kw = dict(min_depth=a.min_depth, min_permille=a.min_permille, edge_clip=a.edge_clip)
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, g_st = kc.align_gapped(d_bases, d_offs, alns)
        depth_ms, depth_kt, _, depth_runs = timed(kc, a.runs, lambda: kc.aln_depths(gaps, edge_clip=a.edge_clip))
        calls = {}
        for name, fixes in (("without_fixes", False), ("with_fixes", True)):
            ms, kt, res, runs = timed(kc, a.runs, lambda: kc.polish_contigs(d_bases, d_offs, gaps, with_records=True, with_fixes=fixes, **kw))
            st = res[4]
            tile_ms = sum(v[1] for n, v in kt.items() if n.startswith("kc_polish_tile_kernel"))
            calls[name] = dict(kernel_ms=round(ms, 4), runs_kernel_ms=runs, over_aln_depths=round(ms / depth_ms, 3) if depth_ms else None,
                               tile_kernel_ms=round(tile_ms, 4), votes_per_s=round(st["votes"] * (2 if fixes else 1) / (tile_ms / 1e3)) if tile_ms else None,
                               kernels={n: dict(launches=v[0], total_ms=round(v[1], 4)) for n, v in kt.items()}, stats=st)
        got = res[0].cpu().numpy()
        restored = int(((got == true_block) & planted).sum())
        wrong = int(((got != block) & (got != true_block)).sum())
        harmed = int(((got != true_block) & ~planted).sum())
        c_ms = copy_ms(2 * len(block), dev)
        out.update(records=gaps.numel() // 32, gap_stats=g_st, aln_depths_kernel_ms=round(depth_ms, 4), aln_depths_runs=depth_runs,
                   aln_depths_kernels={n: dict(launches=v[0], total_ms=round(v[1], 4)) for n, v in depth_kt.items()},
                   block_copy_ms=round(c_ms, 4), calls=calls, over_block_copy=round(calls["without_fixes"]["kernel_ms"] / c_ms, 2) if c_ms else None,
                   planted_restored=restored, restored_share=round(restored / max(int(planted.sum()), 1), 4), bytes_changed_wrongly=wrong,
                   true_bytes_changed=harmed)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
