"""Times kc_close_gaps at the end of a scaffold round on scripts/ctg_links_bench.py's input, with a cutter of its own: every
contig is cut in two and 1 .. 50 bases are REMOVED at the cut, so that the links on record have positive gaps, the walk
leaves N runs, and the reads across the cuts hold what was removed.  The chain is index_contigs -> align_reads ->
align_gapped -> pair_inserts -> ctg_links -> scaffolds -> close_gaps, device tensors throughout.  Prints one JSON line and
writes it to profiles/close_gaps_<date>.json.

Reported: kernel time by pass (HIP events, KC_FLAG_TIME_KERNELS; the median of --runs runs by total kernel time, after one
warm-up), gaps/s and fill bases/s by that time, and, for the writer alone, the time of a device-to-device copy of the same
number of bytes taken in the same run.  Counted, not asserted (the reads carry substitutions at --error-rate): the gaps
filled, the fills equal to the removed piece, the gaps left.  No rate is fixed in advance: there is no earlier version to
compare with, and the host model is a definition, not a baseline."""
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
from mhm2_kmer_analysis_v2_amd import _lib  # noqa: E402
from mhm2_kmer_analysis_v2_amd.kcount import CLOSURE_DTYPE, MEMBER_DTYPE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC = bytes.maketrans(b"ACGT", b"TGCA")


def cut_out(rng, block, offs, margin, max_gap=50):
    """every contig of the block cut at a random point at least margin bases from its ends, with 1 .. max_gap bases removed
    behind the cut: contig u becomes 2u and 2u + 1.  Returns the new block, its offsets, and where in the old block each
    removed piece starts and how long it is."""
    lens = (offs[1:] - offs[:-1]).astype(np.int64) - 1
    g = 1 + (rng.random(len(lens)) * np.minimum(max_gap, lens - 2 * margin - 1)).astype(np.int64)
    cut = margin + (rng.random(len(lens)) * (lens - 2 * margin - g + 1)).astype(np.int64)
    at = offs[:-1].astype(np.int64) + cut
    keep = np.ones(len(block), dtype=bool)
    drop = np.concatenate([np.arange(a + 1, a + n) for a, n in zip(at, g)]) if len(at) else np.zeros(0, np.int64)
    keep[drop] = False  # the first removed byte becomes the separator, the rest go
    new = block.copy()
    new[at] = ord("_")
    new = new[keep]
    new_lens = np.stack([cut, lens - cut - g], axis=1).reshape(-1)
    new_offs = np.zeros(2 * len(lens) + 1, dtype=np.uint64)
    new_offs[1:] = np.cumsum(new_lens + 1)
    return new, new_offs, at, g


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
    ap.add_argument("--min-reads", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "close_gaps_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    whole, whole_offs, bases, roffs, _ = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    block, offs, removed_at, removed_len = cut_out(rng, whole, whole_offs, a.k + 8)
    out = dict(metric="close_gaps", k=a.k, pairs=a.pairs, contigs=2 * a.contigs, cuts=a.contigs, removed_bases=int(removed_len.sum()),
               block_bytes=int(len(block)), error_rate=a.error_rate, min_reads=a.min_reads, host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, _ = kc.align_gapped(d_bases, d_offs, alns)
        _, pairs, _ = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
        links, _, l_st, _ = kc.ctg_links(d_offs, gaps, pairs, insert_avg=int(round(a.frag_mean)), max_insert=a.max_insert, end_slack=a.end_slack)
        _, _, scafs, members, s_st = kc.scaffolds(links)
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            seqs, s_offs, scafs_out, members_out, closures, st = kc.close_gaps(d_bases, d_offs, gaps, scafs, members, min_reads=a.min_reads,
                                                                                end_slack=a.end_slack)
            kt = kc.kernel_times(clear=True)
            if r:
                runs.append((sum(v[1] for v in kt.values()), kt))
        runs.sort(key=lambda x: x[0])
        ms, kt = runs[len(runs) // 2]
        nbytes = int(seqs.numel())
        copy = copy_ms(2 * nbytes, dev)  # a copy of the block's bytes: it reads and writes them once each
        write_ms = kt["kc_close_write_kernel"][1]
        # ---- the fills against what was removed
        text = seqs.cpu().numpy().tobytes()
        mem = members.cpu().numpy().view(MEMBER_DTYPE)
        clo = closures.cpu().numpy().view(CLOSURE_DTYPE)
        whole_text = whole.tobytes()
        at_cut = equal = 0
        for m in np.nonzero(clo["status"] == _lib.KC_CLOSE_FILLED)[0]:
            x, y = mem[m - 1], mem[m]
            u = int(x["ctg"]) >> 1
            forward = int(x["ctg"]) == 2 * u and int(y["ctg"]) == 2 * u + 1 and not x["orient"] and not y["orient"]
            backward = int(x["ctg"]) == 2 * u + 1 and int(y["ctg"]) == 2 * u and x["orient"] and y["orient"]
            if not (forward or backward):
                continue
            at_cut += 1
            piece = whole_text[int(removed_at[u]):int(removed_at[u]) + int(removed_len[u])]
            fill = text[int(clo[m]["fill_pos"]):int(clo[m]["fill_pos"]) + int(clo[m]["new_join"])]
            equal += fill == (piece if forward else piece.translate(RC)[::-1])
        launch_bound = sorted(n for n, v in kt.items() if v[0] and v[1] / v[0] < 0.01)  # under 10 us a launch: the launch, not the bytes
        out.update(link_stats=l_st, scaffold_stats=s_st, close_stats=st, closed_block_bytes=nbytes, kernel_ms=round(ms, 3),
                   runs_kernel_ms=[round(x[0], 3) for x in runs], gaps_per_s=round(st["gaps"] / (ms / 1e3)) if ms else None,
                   fill_bases_per_s=round(st["fill_bases"] / (ms / 1e3)) if ms else None, writer_ms=round(write_ms, 4),
                   copy_of_the_block_ms=round(copy, 4), writer_share_of_copy_rate=round(copy / write_ms, 3), filled=st["filled"],
                   filled_at_a_cut=at_cut, fills_equal_to_the_removed_piece=int(equal), gaps_left=st["gaps"] - st["filled"] - st["abutted"]
                   - st["overlapped"], kernels_under_10us_a_launch=launch_bound,
                   kernels={n: dict(launches=v[0], total_ms=round(v[1], 4)) for n, v in kt.items()})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
