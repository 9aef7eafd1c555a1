"""Times kc_ctg_links behind kc_align_reads, kc_align_gapped and kc_pair_inserts: scripts/depth_insert_bench.py's input
(paired reads of 150 bases cut from random contigs of unitig-like lengths, fragment lengths drawn from a normal
distribution, substitutions planted at an error rate), with every contig cut in two at a random point first, so that reads
and pairs lie across the cuts and links exist.  Prints one JSON line and writes it to profiles/ctg_links_<date>.json.

Reported: candidates/s and links/s by kernel time (HIP events, KC_FLAG_TIME_KERNELS), every kernel's launches and time,
and beside each pass the time a measured device-to-device copy takes for the bytes that pass must move (a copy of n bytes
moves 2n: the pass's reads and writes together are held against a copy of half their sum).  How many of the cuts were
found, and at which gap, is printed beside the rates: a cut is a gap of 0.  No rate is fixed in advance: there is no
earlier version to compare with, and the host model is a definition, not a baseline.
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
from mhm2_kmer_analysis_v2_amd.kcount import LINK_DTYPE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_TILE, SORT_DIGITS, LINK_TILE, SCAN_TILE = 4096, 256, 256, 1024


def cut_in_two(rng, block, offs, margin):
    """every contig of the block cut at a random point at least margin bases from its ends: contig u becomes 2u and 2u + 1"""
    lens = (offs[1:] - offs[:-1]).astype(np.int64) - 1
    cut = margin + (rng.random(len(lens)) * (lens - 2 * margin + 1)).astype(np.int64)
    at = offs[:-1].astype(np.int64) + cut  # the separator goes in front of this byte
    new = np.insert(block, at, ord("_"))
    new_lens = np.stack([cut, lens - cut], axis=1).reshape(-1)
    new_offs = np.zeros(2 * len(lens) + 1, dtype=np.uint64)
    new_offs[1:] = np.cumsum(new_lens + 1)
    return new, new_offs


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
    ap.add_argument("--end-slack", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctg_links_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    block, offs, bases, roffs, f = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    block, offs = cut_in_two(rng, block, offs, a.k + 8)
    nreads = 2 * a.pairs
    out = dict(metric="ctg_links", k=a.k, pairs=a.pairs, read_len=a.read_len, contigs=2 * a.contigs, cuts=a.contigs, block_bytes=int(len(block)),
               error_rate=a.error_rate, insert_avg=int(round(a.frag_mean)), max_insert=a.max_insert, end_slack=a.end_slack,
               host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, g_st = kc.align_gapped(d_bases, d_offs, alns)
        _, pairs, p_st = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
        n = gaps.numel() // 32
        kw = dict(insert_avg=int(round(a.frag_mean)), max_insert=a.max_insert, end_slack=a.end_slack)
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            links, end_first, st, gap = kc.ctg_links(d_offs, gaps, pairs, **kw)
            kt = kc.kernel_times(clear=True)
            if r:
                runs.append((sum(v[1] for v in kt.values()), kt, st))
        runs.sort(key=lambda x: x[0])
        ms, kt, st = runs[len(runs) // 2]
        h = links.cpu().numpy().view(LINK_DTYPE)
        # a cut lies between the right end of contig 2u and the left end of contig 2u + 1: ends 4u + 1 and 4u + 2, gap 0
        at_cut = h[(h["from"] % 4 == 1) & (h["to"] == h["from"] + 1)]
        splinted = at_cut[at_cut["splints"] > 0]
        _, n_ctgs = kc.contig_index_info()
        cands, runs_n = st["splint_cands"] + st["span_cands"], len(h)
        items, units, passed = 2 * cands, nreads + a.pairs, st["passed"]
        tiles, heads = (items + SORT_TILE - 1) // SORT_TILE, (items + LINK_TILE - 1) // LINK_TILE
        rtiles, utiles = (nreads + SCAN_TILE - 1) // SCAN_TILE, (units + SCAN_TILE - 1) // SCAN_TILE
        passes = kt.get("kc_sort_hist_kernel<links>", (0, 0.0))[0]
        # bytes a pass must move: a record is 32 bytes, an offset or a count 8, a slot's summary 16, a key 8, an index or payload 4,
        # a run's figures 48 as they are kept and 48 as they leave
        must = {"kc_align_lengths_kernel<links>": 8 * nreads, "kc_depth_check_kernel<links>": 32 * n + 16 * n,
                "kc_lassm_pair_check_kernel<links>": (16 + 64) * a.pairs, "kc_link_group_kernel<count>": 32 * n + 16 * passed,
                "kc_link_group_kernel<fill>": 32 * n + (8 + 8 + 16 + 8 + 16) * passed,
                "kc_link_tile_scan_kernel": 16 * (nreads + units) + 8 * (rtiles + utiles), "kc_link_scan_kernel": 16 * (rtiles + utiles + heads),
                "kc_link_cands_kernel<count>": 16 * nreads + 16 * passed + (16 + 64 + 16) * a.pairs + 8 * units,
                "kc_link_cands_kernel<write>": 16 * nreads + 16 * passed + (16 + 64 + 16) * a.pairs + 8 * units + 20 * cands,
                "kc_sort_hist_kernel<links>": passes * (8 * items + 8 * SORT_DIGITS * tiles),
                "kc_sort_scan_kernel<links>": passes * 16 * SORT_DIGITS * tiles,
                "kc_sort_scatter_kernel<links>": passes * (24 * items + 8 * SORT_DIGITS * tiles),
                "kc_link_heads_kernel": 8 * items + 8 * heads, "kc_link_reduce_kernel": (8 + 4 + 4) * items + 8 * heads + (8 + 48) * runs_n,
                "kc_link_emit_kernel": (56 + 48) * runs_n, "kc_link_end_first_kernel": 8 * (2 * n_ctgs + 1) + 8 * runs_n}
        kernels = {}
        for name, v in kt.items():
            kernels[name] = dict(launches=v[0], total_ms=round(v[1], 4), bytes_moved=int(must.get(name, 0)),
                                 copy_of_those_bytes_ms=round(copy_ms(must[name], dev), 4) if name in must else None)
        out.update(records=n, gap_stats=g_st, insert_classes=p_st["cls"], link_stats=st, candidates=cands, directed_records=runs_n,
                   kernel_ms=round(ms, 3), runs_kernel_ms=[round(x[0], 3) for x in runs],
                   candidates_per_s=round(cands / (ms / 1e3)) if ms else None, links_per_s=round(st["links"] / (ms / 1e3)) if ms else None,
                   records_per_s=round(n / (ms / 1e3)) if ms else None,
                   cuts_linked=int(len(at_cut)), cuts_splinted=int(len(splinted)), cuts_splinted_at_gap_0=int(
                       ((splinted["splint_gap_min"] == 0) & (splinted["splint_gap_max"] == 0)).sum()),
                   links_not_at_a_cut=int(st["links"] - len(at_cut)), mean_abs_span_gap_at_cuts=round(float(np.abs(
                       at_cut["span_gap_sum"][at_cut["spans"] > 0] / at_cut["spans"][at_cut["spans"] > 0]).mean()), 3) if (at_cut["spans"] > 0).any() else None,
                   kernels=kernels)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
