"""Times kc_ctg_index_build and kc_align_reads on bench.py's synthetic reads (k = 21 by default): the reads are counted, the
unitigs of the results go straight into the seed index on the device, and the same reads are aligned to them, block by
block; prints one JSON line and writes it to profiles/align_reads.json.

Reported: the index statistics and its three kernels; per block of reads one kc_align_reads call with room for two
records a read (count pass, scan, write pass -- no separate size query), its wall time and reads/s, and every kc_align_*
kernel's launches and time (HIP events, KC_FLAG_TIME_KERNELS) summed over the blocks of the run with the median total.
Beside each pass of the reads kernel stands the time a measured device-to-device copy takes for the bytes the pass must
read: the reads' bases and offsets, 8 bytes of slot and k bytes of contig text a window looked up that hits, 8 bytes of
slot a window that does not, and the contig bytes under every record (the overlap is at most the read).  No rate is
fixed in advance.  --runs timed repetitions after one warm-up."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from mhm2_kmer_analysis_v2_amd import _lib  # noqa: E402
from sort_dump_bench import copy_ceiling_gbps, count  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--block", type=int, default=5_000_000, help="reads per kc_align_reads call")
    ap.add_argument("--seed-space", type=int, default=1)
    ap.add_argument("--max-mismatches", type=int, default=_lib.KC_ALIGN_KEEP_ALL)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_reads.json"))
    a = ap.parse_args()
    k, L = a.k, pkg.lib()
    out = dict(metric="align_reads", k=k, reads=a.reads, read_len=a.read_len, block=a.block, seed_space=a.seed_space,
               max_mismatches=a.max_mismatches)
    est_unique = int(64 * 4_000_000 + a.reads * a.read_len * 0.005 * k * 1.05) + (1 << 20)
    with pkg.KmerCounter(k, time_kernels=True, max_elems=est_unique,
                         max_kmers_buffered=int(a.reads * (a.read_len - k - 1) * 1.02) + (1 << 20)) as kc:
        dev = "cuda:%d" % kc.device
        out["results"] = int(count(kc, a.reads, a.reads, a.read_len).n)
        kc.kernel_times(clear=True)
        t0 = time.perf_counter()
        out["index"] = kc.index_unitigs()
        out["index_wall_ms_with_unitigs"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["index_kernels"] = {n: dict(launches=v[0], total_ms=round(v[1], 3)) for n, v in kc.kernel_times(clear=True).items()
                                if n.startswith("kc_align")}
        block = min(a.block, a.reads)
        bases = torch.empty(block * a.read_len, dtype=torch.uint8, device=dev)
        quals = torch.empty_like(bases)
        offs = torch.empty(block + 1, dtype=torch.int64, device=dev)
        alns = torch.empty(2 * block * 32, dtype=torch.uint8, device=dev)
        first = torch.empty(block + 1, dtype=torch.int64, device=dev)
        p = pkg.synth_params(read_len=a.read_len)
        runs, walls, totals = [], [], None
        for r in range(a.runs + 1):  # the first is the warm-up
            kc.kernel_times(clear=True)
            wall, done = 0.0, 0
            tot = dict.fromkeys([n for n, _ in _lib.kc_align_stats._fields_], 0)
            while done < a.reads:
                n = min(block, a.reads - done)
                kc.synth_reads_device(bases, quals, offs, n, first_read=done, params=p)
                torch.cuda.synchronize()
                na, st = C.c_uint64(0), _lib.kc_align_stats()
                t0 = time.perf_counter()
                _lib.check(L.kc_align_reads(kc._h, bases.data_ptr(), offs.data_ptr(), n, 1, a.seed_space, a.max_mismatches, alns.data_ptr(),
                                            2 * block, first.data_ptr(), C.byref(na), C.byref(st)), "kc_align_reads")
                wall += time.perf_counter() - t0
                for f in tot:
                    tot[f] += int(getattr(st, f))
                done += n
            kt = {n: v for n, v in kc.kernel_times(clear=True).items() if n.startswith("kc_align")}
            if r:
                runs.append(kt)
                walls.append(wall)
            totals = tot
        sums = [sum(v[1] for v in kt.values()) for kt in runs]
        mid = sums.index(sorted(sums)[len(sums) // 2])
        med, wall = runs[mid], walls[mid]
        nbases = a.reads * a.read_len
        must_read = (nbases + 8 * (a.reads + 1) + 8 * totals["windows"] + k * (totals["seed_hits"] + totals["repeated_hits"])
                     + a.read_len * totals["alignments"])
        ceiling = copy_ceiling_gbps(min(max(nbases, 1 << 20), 4 << 30), dev)
        copy_ms = 2 * must_read / ceiling / 1e6  # the ceiling counts bytes read + written: a copy of must_read bytes moves twice that
        out.update(stats=totals, wall_ms=round(wall * 1e3, 3), reads_per_s=round(a.reads / wall), runs_kernel_ms=[round(t, 3) for t in sums],
                   pass_must_read_bytes=must_read, copy_ceiling_gbps=round(ceiling, 1), copy_of_those_bytes_ms=round(copy_ms, 3),
                   kernels={n: dict(launches=v[0], total_ms=round(v[1], 3)) for n, v in med.items()})
        for n in ("kc_align_reads_kernel<count>", "kc_align_reads_kernel<write>"):
            if n in med and med[n][1]:
                out["kernels"][n]["times_the_copy"] = round(med[n][1] / copy_ms, 2)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
