"""Times kc_sort_results and kc_dump_text_device on the results of a full-size count, beside the host path they replace,
and prints one JSON line.

Device: the number of results; the sort's kernels (HIP events, KC_FLAG_TIME_KERNELS) in total, by kernel and per pass
(a pass is one histogram, one scan, one scatter; the passes of a word move the same bytes, so a kernel's total over its
launches is what is reported, and the average); the bytes a pass must move -- n x (8 key bytes carried + 4) read and
written by the scatter, n x 8 read by the histogram, and the digit counters written, scanned and read -- and that as a
fraction of a measured device-to-device copy; the text rate per chunk of 2^24 lines.
Host, in the same run: kc_copy_results + np.lexsort in full, and the Python line formatting on the first 10^6 lines,
reported per line.

The sort cannot be repeated on one context (a second call does nothing), so every repetition counts again:
--runs of them after one warm-up, the median reported."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from mhm2_kmer_analysis_v2_amd.kcount import kmer_to_string  # noqa: E402

SORT_TILE, SORT_DIGITS, SORT_BITS = 4096, 256, 8


def passes_of(k):
    n = 0
    for w in range(k // 32, -1, -1):
        sig = max(0, min(64, 2 * k - 64 * w))
        n += (sig + SORT_BITS - 1) // SORT_BITS
    return n


def count(kc, reads, block, read_len):
    dev = "cuda:%d" % kc.device
    bases = torch.empty(block * read_len, dtype=torch.uint8, device=dev)
    quals = torch.empty_like(bases)
    offs = torch.empty(block + 1, dtype=torch.int64, device=dev)
    p = pkg.synth_params(read_len=read_len)
    done = 0
    while done < reads:
        n = min(block, reads - done)
        kc.synth_reads_device(bases, quals, offs, n, first_read=done, params=p)
        kc.submit_reads(bases, quals, offs, nreads=n)
        done += n
    kc.flush()
    return kc.finalize()


def copy_ceiling_gbps(nbytes, device):
    a = torch.empty(nbytes, dtype=torch.uint8, device=device)
    b = torch.empty_like(a)
    ms = []
    for r in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return 2 * nbytes / statistics.median(ms) / 1e6  # read + written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--block", type=int, default=0, help="reads per submit (0: all at once, as bench.py does)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk-lines", type=int, default=1 << 24)
    a = ap.parse_args()
    k = a.k
    npass = passes_of(k)
    out = dict(metric="sort_dump", k=k, reads=a.reads, passes=npass)
    # sized as bench.py sizes its counter: the genomes' k-mers and about k per substitution error
    est_unique = int(64 * 4_000_000 + a.reads * a.read_len * 0.005 * k * 1.05) + (1 << 20)
    with pkg.KmerCounter(k, time_kernels=True, max_elems=est_unique,
                         max_kmers_buffered=int(a.reads * (a.read_len - k - 1) * 1.02) + (1 << 20)) as kc:
        sort_runs, wall_runs = [], []
        for r in range(a.runs + 1):  # the first run is the warm-up
            if r:
                kc.reset()
            n = int(count(kc, a.reads, a.block or a.reads, a.read_len).n)
            if r == 0:  # the host path, on the unsorted results the parent commit offers
                t0 = time.perf_counter()
                keys, counts, left, right = kc.results()
                t1 = time.perf_counter()
                order = np.lexsort([keys[:, j] for j in range(kc.nl - 1, -1, -1)])
                keys, counts, left, right = keys[order], counts[order], left[order], right[order]
                t2 = time.perf_counter()
                m = min(n, 1_000_000)
                lines = ["%s %d %s %s" % (kmer_to_string(keys[i], k), counts[i], chr(left[i]), chr(right[i])) for i in range(m)]
                t3 = time.perf_counter()
                out["host"] = dict(copy_results_s=round(t1 - t0, 3), lexsort_and_reorder_s=round(t2 - t1, 3), format_lines=m,
                                   format_us_per_line=round((t3 - t2) / max(m, 1) * 1e6, 3))
                head = "".join(x + "\n" for x in lines[:1000]).encode()
                del keys, counts, left, right, order, lines
            kc.kernel_times(clear=True)
            t0 = time.perf_counter()
            kc.sort_results()
            wall = (time.perf_counter() - t0) * 1e3
            kt = {name: v for name, v in kc.kernel_times(clear=True).items() if name.startswith("kc_sort")}
            if r:
                sort_runs.append(kt)
                wall_runs.append(wall)
        tot = [sum(v[1] for v in kt.values()) for kt in sort_runs]
        med = sort_runs[tot.index(sorted(tot)[len(tot) // 2])]
        ntiles = (n + SORT_TILE - 1) // SORT_TILE
        pass_bytes = n * 8 + 2 * n * 12 + 3 * ntiles * SORT_DIGITS * 8 + ntiles * SORT_DIGITS * 8
        ceiling = copy_ceiling_gbps(min(max(n * 12, 1 << 20), 4 << 30), "cuda:%d" % kc.device)
        pass_ms = sum(med[x][1] for x in med if "gather" not in x) / npass
        out["results"] = n
        out["sort"] = dict(total_ms=round(sum(v[1] for v in med.values()), 3), wall_ms=round(statistics.median(wall_runs), 3),
                           kernels={name: dict(launches=v[0], total_ms=round(v[1], 3)) for name, v in med.items()},
                           per_pass_ms=round(pass_ms, 3), pass_bytes=pass_bytes,
                           pass_gbps=round(pass_bytes / pass_ms / 1e6, 1) if pass_ms else None,
                           copy_ceiling_gbps=round(ceiling, 1),
                           fraction_of_copy_ceiling=round(pass_bytes / pass_ms / 1e6 / ceiling, 3) if pass_ms else None,
                           runs_total_ms=[round(t, 3) for t in tot])
        # the text, chunk by chunk into one device buffer (the copy to the host is not part of the rate)
        assert kc.dump_text(0, min(n, 1000)) == head  # the two paths agree on the first lines
        import ctypes as C
        L = pkg.lib()
        chunks = []
        cap = (k + 11) * min(a.chunk_lines, n)  # a line: k + 5 + up to five digits, and the newline
        buf = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda:%d" % kc.device)
        torch.cuda.synchronize()
        for rep in range(2):  # the first sweep is the warm-up
            chunks = []
            for first in range(0, n, a.chunk_lines):
                c = min(a.chunk_lines, n - first)
                kc.kernel_times(clear=True)
                nb = C.c_uint64(0)
                pkg._lib.check(L.kc_dump_text_device(kc._h, first, c, buf.data_ptr(), cap, C.byref(nb)), "kc_dump_text_device")
                kt = kc.kernel_times(clear=True)
                ms = sum(v[1] for name, v in kt.items() if name.startswith("kc_dump"))
                chunks.append(dict(lines=c, bytes=nb.value, ms=round(ms, 3), gbps=round(nb.value / ms / 1e6, 1) if ms else None))
        out["text"] = dict(chunk_lines=a.chunk_lines, chunks=chunks[:8], nchunks=len(chunks), total_bytes=sum(c["bytes"] for c in chunks),
                           median_gbps=statistics.median([c["gbps"] for c in chunks if c["gbps"]]) if chunks else None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
