"""Times kc_build_unitigs on the results of a count of bench.py's synthetic reads (k = 21 by default), kernel by kernel,
beside a measured device copy of the same bytes; prints one JSON line and writes it to profiles/unitigs.json.

Per kernel (HIP events, KC_FLAG_TIME_KERNELS): launches and total time of a size query and the call that follows it, which
is what KmerCounter.unitigs() does: everything up to the scan runs twice (links, the rounds of the cycle search, the cut,
the rounds of the ranking, selection, scan), write and depths once.  The bytes a round of pointer jumping must
move are 2n nodes x 8 bytes (pointer + carried value) read, as many gathered through the pointer, and as many written:
3 x 16n bytes; that over the measured time of a round, as a fraction of a device-to-device copy, is reported for both
jumping kernels.  The results are sorted before the timed call, so the sort (scripts/sort_dump_bench.py) is not in it.
--runs timed calls after one warm-up, the one with the median total reported."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from sort_dump_bench import copy_ceiling_gbps, count  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--block", type=int, default=0, help="reads per submit (0: all at once, as bench.py does)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitigs.json"))
    a = ap.parse_args()
    k = a.k
    out = dict(metric="unitigs", k=k, reads=a.reads)
    est_unique = int(64 * 4_000_000 + a.reads * a.read_len * 0.005 * k * 1.05) + (1 << 20)
    with pkg.KmerCounter(k, time_kernels=True, max_elems=est_unique,
                         max_kmers_buffered=int(a.reads * (a.read_len - k - 1) * 1.02) + (1 << 20)) as kc:
        n = int(count(kc, a.reads, a.block or a.reads, a.read_len).n)
        kc.sort_results()
        runs, walls, st = [], [], None
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            t0 = time.perf_counter()
            seqs, depths, offsets, sums, st = kc._unitigs(True, True)
            walls.append((time.perf_counter() - t0) * 1e3)
            kt = {name: v for name, v in kc.kernel_times(clear=True).items() if name.startswith("kc_unitig")}
            if r:
                runs.append(kt)
            del seqs, depths, offsets, sums
        tot = [sum(v[1] for v in kt.values()) for kt in runs]
        med = runs[tot.index(sorted(tot)[len(tot) // 2])]
        rounds = (2 * n - 1).bit_length() + 1 if n else 0
        round_bytes = 3 * 16 * n
        ceiling = copy_ceiling_gbps(min(max(16 * n, 1 << 20), 4 << 30), "cuda:%d" % kc.device)
        out.update(results=n, stats=st, rounds=rounds, round_bytes=round_bytes, copy_ceiling_gbps=round(ceiling, 1),
                   total_ms=round(sum(v[1] for v in med.values()), 3), wall_ms_query_and_call=round(sorted(walls[1:])[len(walls[1:]) // 2], 3),
                   runs_total_ms=[round(t, 3) for t in tot],
                   kernels={name: dict(launches=v[0], total_ms=round(v[1], 3)) for name, v in med.items()})
        for name in ("kc_unitig_min_jump_kernel", "kc_unitig_rank_jump_kernel"):
            if name in med and med[name][1]:
                per = med[name][1] / med[name][0]
                out["kernels"][name].update(per_round_ms=round(per, 4), round_gbps=round(round_bytes / per / 1e6, 1),
                                            fraction_of_copy_ceiling=round(round_bytes / per / 1e6 / ceiling, 3))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
