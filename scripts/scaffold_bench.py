"""Times kc_scaffold behind kc_ctg_links on scripts/ctg_links_bench.py's input: contigs of unitig-like lengths each cut in
two at a random point, paired reads across the cuts, so that the links on record are the cuts and the walk has to put every
contig together again.  Prints one JSON line and writes it to profiles/scaffold_<date>.json.

Reported: kernel time by pass (HIP events, KC_FLAG_TIME_KERNELS; the median of --runs runs by total kernel time, after one
warm-up), scaffolds/s and block bytes/s by that time, and, for the writer alone, the time of a device-to-device copy of the
same number of bytes taken in the same run.  The by-construction claims are checked and counted: a scaffold whose joins
are all 0 must equal the uncut contig it came from, and no scaffold may join pieces of different contigs.  No rate is fixed
in advance: there is no earlier version to compare with, and the host model is a definition, not a baseline."""
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
from ctg_links_bench import cut_in_two  # noqa: E402
from depth_insert_bench import copy_ms, make_input  # noqa: E402
from mhm2_kmer_analysis_v2_amd.kcount import MEMBER_DTYPE, SCAFFOLD_DTYPE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--overlap-slack", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaffold_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    whole, whole_offs, bases, roffs, _ = make_input(rng, a.pairs, a.read_len, a.contigs, a.error_rate, a.frag_mean, a.frag_sd)
    block, offs = cut_in_two(rng, whole, whole_offs, a.k + 8)
    out = dict(metric="scaffold", k=a.k, pairs=a.pairs, contigs=2 * a.contigs, cuts=a.contigs, block_bytes=int(len(block)),
               overlap_slack=a.overlap_slack, host_input_s=round(time.perf_counter() - t0, 1))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        kc.index_contigs(torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
        d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(roffs.view(np.int64)).to(dev)
        alns, _, _ = kc.align_reads(d_bases, d_offs)
        gaps, _ = kc.align_gapped(d_bases, d_offs, alns)
        _, pairs, _ = kc.pair_inserts(d_offs, gaps, max_insert=a.max_insert)
        links, _, l_st, _ = kc.ctg_links(d_offs, gaps, pairs, insert_avg=int(round(a.frag_mean)), max_insert=a.max_insert, end_slack=a.end_slack)
        runs = []
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            seqs, s_offs, scafs, members, st = kc.scaffolds(links, overlap_slack=a.overlap_slack)
            kt = kc.kernel_times(clear=True)
            if r:
                runs.append((sum(v[1] for v in kt.values()), kt))
        runs.sort(key=lambda x: x[0])
        ms, kt = runs[len(runs) // 2]
        nbytes = int(seqs.numel())
        copy = copy_ms(2 * nbytes, dev)  # a copy of the block's bytes: it reads and writes them once each
        write_ms = kt["kc_scaf_write_kernel"][1]
        # ---- the claims of the construction
        text = seqs.cpu().numpy().tobytes()
        so = s_offs.cpu().numpy()
        sc = scafs.cpu().numpy().view(SCAFFOLD_DTYPE)
        mem = members.cpu().numpy().view(MEMBER_DTYPE)
        whole_text = whole.tobytes()
        mixed = joined = joined_at_0 = equal_uncut = 0
        for i, s in enumerate(sc):
            if s["n_members"] == 1:
                continue
            m = mem[int(s["first_member"]):int(s["first_member"]) + int(s["n_members"])]
            joined += 1
            if len(set(int(x) >> 1 for x in m["ctg"])) != 1:
                mixed += 1
                continue
            if (m["join"] == 0).all():
                joined_at_0 += 1
                u = int(m["ctg"][0]) >> 1
                want = whole_text[int(whole_offs[u]):int(whole_offs[u + 1]) - 1]
                equal_uncut += text[int(so[i]):int(so[i + 1]) - 1] == want
        if mixed or equal_uncut != joined_at_0:
            raise SystemExit("the construction's claims do not hold: %d scaffolds join different contigs, %d of %d joined at 0 equal their contig"
                             % (mixed, equal_uncut, joined_at_0))
        launch_bound = sorted(n for n, v in kt.items() if v[0] and v[1] / v[0] < 0.01)  # under 10 us a launch: the launch, not the bytes
        out.update(link_records=int(links.numel() // 48), links=l_st["links"], scaffold_stats=st, scaffold_block_bytes=nbytes,
                   kernel_ms=round(ms, 3), runs_kernel_ms=[round(x[0], 3) for x in runs],
                   scaffolds_per_s=round(st["scaffolds"] / (ms / 1e3)), block_bytes_per_s=round(nbytes / (ms / 1e3)),
                   writer_ms=round(write_ms, 4), copy_of_the_block_ms=round(copy, 4), writer_share_of_copy_rate=round(copy / write_ms, 3),
                   scaffolds_joined=joined, joined_with_every_join_0=joined_at_0, of_those_equal_to_the_uncut_contig=equal_uncut,
                   scaffolds_joining_different_contigs=mixed, kernels_under_10us_a_launch=launch_bound,
                   kernels={n: dict(launches=v[0], total_ms=round(v[1], 4)) for n, v in kt.items()})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
