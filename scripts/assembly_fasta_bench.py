"""Times kc_ctg_select and kc_fasta_text on two blocks: the 40 000-contig block scripts/scaffold_bench.py builds, and a
synthetic block of about a gigabyte with heavy-tailed lengths (21 .. 20 M bases, from a seed), made on the device.  Prints one
JSON line and writes it to profiles/assembly_fasta_<date>.json.

Reported, per block: kc_ctg_select's kernels (HIP events, KC_FLAG_TIME_KERNELS), and for line widths 0, 60 and 80 the
writer's kernel time -- the median of --runs whole-text calls after a warm-up -- as bytes written over that time, beside the
time and rate of a device-to-device copy that moves the same number of bytes (it reads and writes them once each), made in
the same run: that copy is the yardstick, no ratio chosen in advance.  Beside it, for information, what the calls replace:
the wall time of _block_strings and a join of the records on the host, on the same block.  A window of the device's text
is compared with the host's.  Needs a GPU: there is no fallback."""
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
from mhm2_kmer_analysis_v2_amd.kcount import _block_strings  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (0, 60, 80)


def scaffold_bench_block(dev):
    """the 40 000 contigs scaffold_bench.py cuts its 20 000 in, at its defaults"""
    rng = np.random.default_rng(1)
    whole, whole_offs, _, _, _ = make_input(rng, 400_000, 150, 20000, 0.005, 400.0, 50.0)
    block, offs = cut_in_two(rng, whole, whole_offs, 21 + 8)
    return torch.from_numpy(block).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev)


def heavy_block(dev, seed, nbytes):
    """contigs of min(20 M, 21 + floor(200 Pareto(1))) bases until the block has nbytes, random ACGT with an N in a thousand"""
    rng = np.random.default_rng(seed)
    lengths = np.minimum(20_000_000, 21 + np.floor(200 * rng.pareto(1.0, size=nbytes // 400))).astype(np.int64)
    ends = np.cumsum(lengths + 1)
    n = int(np.searchsorted(ends, nbytes, side="right"))
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = ends[:n]
    total = int(offs[-1])
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    seqs = torch.empty(total, dtype=torch.uint8, device=dev)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    for at in range(0, total, 1 << 26):  # in pieces: the 64-bit indices of a gigabyte at once would be eight
        codes = torch.randint(0, 4000, (min(1 << 26, total - at),), generator=gen, device=dev)
        piece = letters[codes & 3]
        piece[codes >= 3996] = ord("N")
        seqs[at:at + len(piece)] = piece
    d_offs = torch.from_numpy(offs).to(dev)
    seqs[d_offs[1:] - 1] = ord("_")
    return seqs, d_offs


def timed(kc, runs, call):
    """(median total kernel ms, that run's {kernel: (launches, ms)}, all totals, the last result) of `call`, after one warm-up"""
    got, res = [], None
    for r in range(runs + 1):
        kc.kernel_times(clear=True)
        res = call()
        kt = kc.kernel_times(clear=True)
        if r:
            got.append((sum(v[1] for v in kt.values()), kt))
    got.sort(key=lambda x: x[0])
    return got[len(got) // 2] + ([round(x[0], 3) for x in got], res)


def measure(kc, name, seqs, offs, min_len, runs, host_side):
    dev = seqs.device
    nbytes, n = int(seqs.numel()), int(offs.numel()) - 1
    out = dict(block=name, contigs=n, block_bytes=nbytes, min_len=min_len)
    ms, kt, all_ms, (order, st) = timed(kc, runs, lambda: kc.select_contigs(seqs, offs, min_len=min_len, by_length=True))
    comp = kt.get("kc_asm_comp_kernel", (0, 0.0))[1]
    out.update(select_kernel_ms=round(ms, 3), select_runs_kernel_ms=all_ms, select_stats=st,
               comp_ms=round(comp, 4), comp_bytes_per_s=round(nbytes / (comp / 1e3)) if comp else None,
               select_kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()})
    print(pkg.format_assembly_stats(st, min_len), file=sys.stderr)
    widths = {}
    for width in WIDTHS:
        call_text = kc._fasta_call(seqs, offs, order, "scaffold_", width)[0]
        total = call_text(0, None, 0)[1]
        text = torch.empty(total, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms, kt, all_ms, (written, _) = timed(kc, runs, lambda: call_text(0, text.data_ptr(), total))
        assert written == total
        w_ms = kt["kc_asm_write_kernel"][1]
        copy = copy_ms(2 * total, dev)
        widths[str(width)] = dict(text_bytes=total, call_kernel_ms=round(ms, 3), runs_kernel_ms=all_ms, writer_ms=round(w_ms, 4),
                                  writer_bytes_written_per_s=round(total / (w_ms / 1e3)), copy_of_those_bytes_ms=round(copy, 4),
                                  copy_bytes_written_per_s=round(total / (copy / 1e3)), writer_share_of_copy_rate=round(copy / w_ms, 3),
                                  kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()})
        if width == 60:  # a window of the device's text against the host's, from the middle of it
            first = total // 2
            got = text[first:first + (1 << 20)].cpu().numpy().tobytes()
            t0 = time.perf_counter()
            streamed = kc.fasta_text(seqs, offs, order, line_width=60, first_byte=first, capacity=1 << 20)
            widths["60"]["one_MiB_window_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            if streamed != got:
                raise SystemExit("%s: a window of the text differs from the same bytes of the whole" % name)
        del text
    out["widths"] = widths
    if host_side:
        t0 = time.perf_counter()
        strings = _block_strings(seqs, offs)
        host = "".join(">scaffold_%d\n%s\n" % (u, strings[u]) for u in order.cpu().tolist()).encode()
        out["host_block_strings_and_join_wall_s"] = round(time.perf_counter() - t0, 3)
        if host != kc.fasta_text(seqs, offs, order):
            raise SystemExit("%s: the device's text at width 0 differs from the host's" % name)
        out["width_0_equals_the_host_text"] = True
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--heavy-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--min-len", type=int, default=500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assembly_fasta_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("assembly_fasta_bench.py needs a GPU: the HIP path is the only path")
    out = dict(metric="assembly_fasta", seed=a.seed, runs=a.runs, blocks=[])
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        t0 = time.perf_counter()
        seqs, offs = scaffold_bench_block(dev)
        out["host_input_s"] = round(time.perf_counter() - t0, 1)
        out["blocks"].append(measure(kc, "scaffold_bench", seqs, offs, 0, a.runs, True))
        del seqs, offs
        seqs, offs = heavy_block(dev, a.seed, a.heavy_bytes)
        out["blocks"].append(measure(kc, "heavy_tailed", seqs, offs, a.min_len, a.runs, True))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
