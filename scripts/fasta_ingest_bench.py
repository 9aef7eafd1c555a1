"""Times kc_fasta_to_block on three texts: the heavy-tailed block of scripts/assembly_fasta_bench.py (about a gigabyte, contigs
of 21 .. 20 M bases) written by kc_fasta_text at line width 0 and at width 60, and a text of many small contigs (20 .. 59
bases, a depth in every header).  Prints one JSON line and writes it to profiles/fasta_ingest_<date>.json.

Reported, per text: the call's kernel time per kernel (HIP events, KC_FLAG_TIME_KERNELS) -- the median of --runs calls after a
warm-up, into arrays sized by a size query -- and the text's bytes over that time.  Beside it, from the same run, three rates
for comparison, none chosen in advance: a device-to-device copy of the same bytes, kc_fastq_to_packed_device on a FASTQ text
of the same size, and the host path the call replaces, a plain Python FASTA reader that builds the block (on a prefix of at
most --host-bytes).  The round trip is checked: kc_fasta_text then kc_fasta_to_block gives the block and its offsets back
exactly.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
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
from assembly_fasta_bench import heavy_block, timed  # noqa: E402
from depth_insert_bench import copy_ms  # noqa: E402
from mhm2_kmer_analysis_v2_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_text(kc, seqs, offs, width):
    """the whole text of a block on the device, in one window"""
    call = kc._fasta_call(seqs, offs, None, "scaffold_", width)[0]
    total = call(0, None, 0)[1]
    text = torch.empty(total, dtype=torch.uint8, device=seqs.device)
    torch.cuda.synchronize()
    assert call(0, text.data_ptr(), total)[0] == total
    return text


def small_contigs_text(seed, n):
    """n contigs of 20 .. 59 bases in one line each, ">Contig<j> <depth>" in front"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(20, 60, size=n)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(lengths.sum()))].tobytes()
    ends = np.cumsum(lengths)
    return b"".join(b">Contig%d %d.5\n%s\n" % (j, j % 300, bases[e - l:e]) for j, (l, e) in enumerate(zip(lengths.tolist(), ends.tolist())))


def fastq_text(dev, seed, nbytes):
    """a FASTQ text of about nbytes: 2048 seeded records of 150 bases, repeated"""
    rng = np.random.default_rng(seed)
    recs = []
    for j in range(2048):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=150)].tobytes()
        recs.append(b"@r%d\n%s\n+\n%s\n" % (j, s, b"I" * 150))
    unit = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).to(dev)
    return unit.repeat(max(1, nbytes // unit.numel()))


def host_reader(text):
    """what the call replaces: FASTA text -> (block, offsets) in plain Python"""
    seqs, cur = [], None
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r \t")
        if line[:1] == b">":
            cur = []
            seqs.append(cur)
        elif line:
            cur.append(line.upper())
    joined = [b"".join(s) for s in seqs]
    offsets = np.zeros(len(joined) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) + 1 for s in joined])
    return np.frombuffer(b"_".join(joined) + b"_", dtype=np.uint8), offsets


def measure(kc, name, text, runs, host_bytes, want=None):
    dev, n = text.device, int(text.numel())
    L = pkg.lib()
    prm = _lib.kc_fasta_in_params(0, 0)
    nc, nb, cons, st = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), _lib.kc_fasta_in_stats()

    def call(seqs=None, offs=None, cap_b=0, cap_c=0):
        pkg.kcount.check(L.kc_fasta_to_block(kc._h, text.data_ptr(), n, 1, C.byref(prm), seqs, cap_b, offs, cap_c, None, None, C.byref(nc), C.byref(nb),
                                             C.byref(cons), C.byref(st)), "kc_fasta_to_block")

    torch.cuda.synchronize()
    call()  # the size query
    n_ctgs, nbytes = int(nc.value), int(nb.value)
    seqs = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    offs = torch.empty(n_ctgs + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ms, kt, all_ms, _ = timed(kc, runs, lambda: call(seqs.data_ptr(), offs.data_ptr(), nbytes, n_ctgs))
    copy = copy_ms(2 * n, dev)
    out = dict(text=name, text_bytes=n, contigs=n_ctgs, block_bytes=nbytes, stats=pkg.kcount._stats_dict(st), call_kernel_ms=round(ms, 3),
               runs_kernel_ms=all_ms, text_bytes_per_s=round(n / (ms / 1e3)), copy_of_those_bytes_ms=round(copy, 4),
               copy_bytes_per_s=round(n / (copy / 1e3)), share_of_copy_rate=round(copy / ms, 3),
               kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()})
    if want is not None:
        if not (torch.equal(seqs, want[0]) and torch.equal(offs, want[1])):
            raise SystemExit("%s: the block does not come back from its own text" % name)
        out["round_trip_exact"] = True
    # the FASTQ parser on a text of the same size
    fq = fastq_text(dev, 3, n)
    packed, fo = torch.empty(fq.numel(), dtype=torch.uint8, device=dev), torch.empty(fq.numel() // 4 + 2, dtype=torch.int64, device=dev)
    nr, nbq, cq = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    torch.cuda.synchronize()
    fms, fkt, fall, _ = timed(kc, runs, lambda: pkg.kcount.check(L.kc_fastq_to_packed_device(
        kc._h, fq.data_ptr(), fq.numel(), 1, 0, packed.data_ptr(), fq.numel(), fo.data_ptr(), fq.numel() // 4 + 1, C.byref(nr), C.byref(nbq),
        C.byref(cq)), "kc_fastq_to_packed_device"))
    fcopy = copy_ms(2 * fq.numel(), dev)
    out["fastq_same_size"] = dict(text_bytes=int(fq.numel()), reads=int(nr.value), call_kernel_ms=round(fms, 3), runs_kernel_ms=fall,
                                  text_bytes_per_s=round(fq.numel() / (fms / 1e3)), share_of_copy_rate=round(fcopy / fms, 3))
    del fq, packed, fo
    # the host path, on a prefix that ends in front of a header
    prefix = text[:min(n, host_bytes)].cpu().numpy().tobytes()
    if len(prefix) < n:
        prefix = prefix[:prefix.rfind(b"\n>") + 1]
    t0 = time.perf_counter()
    h_seqs, h_offs = host_reader(prefix)
    wall = time.perf_counter() - t0
    out["host_python_reader"] = dict(text_bytes=len(prefix), wall_s=round(wall, 3), text_bytes_per_s=round(len(prefix) / wall))
    k = len(h_offs) - 1
    if not (np.array_equal(h_offs.view(np.int64), offs[:k + 1].cpu().numpy()) and np.array_equal(h_seqs, seqs[:int(h_offs[-1])].cpu().numpy())):
        raise SystemExit("%s: the device's block differs from the host reader's on the prefix" % name)
    out["host_prefix_equal"] = True
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--heavy-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--small-contigs", type=int, default=4_000_000)
    ap.add_argument("--host-bytes", type=int, default=64 << 20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_ingest_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("fasta_ingest_bench.py needs a GPU: the HIP path is the only path")
    out = dict(metric="fasta_ingest", seed=a.seed, runs=a.runs, texts=[])
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        seqs, offs = heavy_block(dev, a.seed, a.heavy_bytes)
        for width in (0, 60):
            text = block_text(kc, seqs, offs, width)
            out["texts"].append(measure(kc, "heavy_tailed_width_%d" % width, text, a.runs, a.host_bytes, (seqs, offs)))
            del text
        del seqs, offs
        text = torch.from_numpy(np.frombuffer(small_contigs_text(a.seed, a.small_contigs), dtype=np.uint8).copy()).to(dev)
        out["texts"].append(measure(kc, "small_contigs", text, a.runs, a.host_bytes))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
