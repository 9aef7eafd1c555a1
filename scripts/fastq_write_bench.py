"""Times kc_fastq_text on two sets of reads: 400 000 pairs of 150 bases (synth_reads_device) and 4 M reads of 20 .. 59 bases,
each as ASCII reads and as the read cache's packed bytes, written as pairs in one window.  Prints one JSON line and writes
it to profiles/fastq_write_<date>.json.

Reported, per case: the call's kernel time per kernel (HIP events, KC_FLAG_TIME_KERNELS) -- the median of --runs calls after a
warm-up, into a buffer sized by a size query -- the text's bytes over that time and over the writer's own time, and the ratio to
a device-to-device copy of the same bytes in the same run.  Beside it: which path the text's sixteen-byte chunks took, counted
on the host from the records' lengths (inside a base line, inside a quality line, over the join of the two, over a name line
or a record's end), and the host path the call replaces, a plain Python formatting of the same reads after a device-to-host
copy (at most --host-reads of them).  The text is checked: a prefix against the Python formatting, the whole through
kc_fastq_pairs_device (ASCII) or kc_fastq_to_packed_device (packed) against the reads.  Needs a GPU: there is no fallback."""
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
from assembly_fasta_bench import timed  # noqa: E402
from depth_insert_bench import copy_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth_reads(kc, dev, nreads, read_len):
    bases = torch.empty(nreads * read_len, dtype=torch.uint8, device=dev)
    quals = torch.empty(nreads * read_len, dtype=torch.uint8, device=dev)
    offs = torch.empty(nreads + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    kc.synth_reads_device(bases, quals, offs, nreads, params=pkg.synth_params(read_len=read_len, n_rate=0.001))
    torch.cuda.synchronize()
    return bases, quals, offs


def short_reads(dev, seed, nreads):
    """reads of 20 .. 59 bases: ACGT, qualities '#' .. 'I'"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lens = torch.randint(20, 60, (nreads,), generator=g, device=dev)
    offs = torch.zeros(nreads + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(lens, 0)
    n = int(offs[-1])
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n,), generator=g, device=dev)]
    quals = torch.randint(35, 74, (n,), generator=g, device=dev).to(torch.uint8)
    return bases, quals, offs


def pack(bases, quals):
    """the read cache's bytes of ASCII reads (code | min(quality - 33, 31) << 3), by torch on the device"""
    code = torch.full((256,), 4, dtype=torch.uint8, device=bases.device)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    q = torch.clamp(quals.to(torch.int16) - 33, 0, 31).to(torch.uint8)
    return code[bases.long()] | (q << 3)


def chunk_paths(lens, prefix_len=1):
    """how many aligned sixteen-byte chunks of the paired text lie in a base line, in a quality line, over the join of the
    two, and anywhere else (a name line or a record's end in it: record by record), from the reads' lengths alone"""
    i = np.arange(len(lens), dtype=np.int64)
    digits = np.char.str_len((i - (i & 1)).astype(str)).astype(np.int64)
    hdr = 2 + prefix_len + digits + 2
    size = hdr + 2 * lens + 4
    start = np.cumsum(size) - size

    def whole(a, b):  # aligned chunks inside [a, b)
        first = (a + 15) // 16 * 16
        return np.maximum((b - first) // 16, 0)

    body = whole(start + hdr, start + size - 1)
    base = whole(start + hdr, start + hdr + lens)
    qual = whole(start + hdr + lens + 3, start + size - 1)
    total = (int(size.sum()) + 15) // 16
    fast = int(body.sum())
    return dict(chunks=total, base_line=int(base.sum()), quality_line=int(qual.sum()), join=fast - int(base.sum()) - int(qual.sum()),
                record_by_record=total - fast)


def host_format(bases, quals, offs, nreads, packed):
    """what the call replaces: a device-to-host copy and plain Python formatting"""
    t0 = time.perf_counter()
    end = int(offs[nreads])
    b, o = bases[:end].cpu().numpy(), offs[:nreads + 1].cpu().numpy()
    if packed:
        q = ((b >> 3) + 33).astype(np.uint8).tobytes()
        b = np.frombuffer(b"ACGTNNNN", dtype=np.uint8)[b & 7].tobytes()
    else:
        b, q = b.tobytes(), quals[:end].cpu().numpy().tobytes()
    o = o.tolist()
    text = b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i - (i & 1), 1 + (i & 1), b[o[i]:o[i + 1]], q[o[i]:o[i + 1]]) for i in range(nreads))
    return text, time.perf_counter() - t0


def measure(kc, name, bases, quals, offs, packed, runs, host_reads):
    dev, nreads = bases.device, int(offs.numel()) - 1
    src = pack(bases, quals) if packed else bases
    call = kc._fastq_call(src, None if packed else quals, offs, None, None, "r", True, 0, None)[0]
    torch.cuda.synchronize()
    total = call(0, None, 0)[1]
    text = torch.empty(total, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ms, kt, all_ms, res = timed(kc, runs, lambda: call(0, text.data_ptr(), total))
    assert res == (total, total)
    write = kt["kc_rtext_write_kernel"][1]
    copy = copy_ms(2 * total, dev)
    out = dict(case=name, reads=nreads, source_bytes=int(src.numel()) * (1 if packed else 2), text_bytes=total, call_kernel_ms=round(ms, 3),
               runs_kernel_ms=all_ms, text_bytes_per_s=round(total / (ms / 1e3)), writer_ms=round(write, 4),
               writer_text_bytes_per_s=round(total / (write / 1e3)), copy_of_those_bytes_ms=round(copy, 4),
               copy_bytes_per_s=round(total / (copy / 1e3)), share_of_copy_rate=round(copy / ms, 3), writer_share_of_copy_rate=round(copy / write, 3),
               chunk_paths=chunk_paths(np.diff(offs.cpu().numpy())),
               kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()})
    # the host path, and the text against it
    k = min(nreads, host_reads) & ~1
    want, wall = host_format(src, quals, offs, k, packed)
    if text[:len(want)].cpu().numpy().tobytes() != want:
        raise SystemExit("%s: the device's text differs from the Python formatting" % name)
    out["host_python_format"] = dict(reads=k, text_bytes=len(want), wall_s=round(wall, 3), text_bytes_per_s=round(len(want) / wall))
    # ... and back through the device's parser
    if packed:
        p2, o2 = kc.fastq_to_packed(text)
        same = torch.equal(p2, src) and torch.equal(o2, offs)
    else:
        b2, q2, o2 = kc.fastq_pairs(text)
        same = torch.equal(b2, bases) and torch.equal(q2, quals) and torch.equal(o2, offs)
    if not same:
        raise SystemExit("%s: the reads do not come back from their own text" % name)
    out["round_trip_exact"] = True
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=400_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--short-reads", type=int, default=4_000_000)
    ap.add_argument("--host-reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_write_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("fastq_write_bench.py needs a GPU: the HIP path is the only path")
    out = dict(metric="fastq_write", seed=a.seed, runs=a.runs, cases=[])
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        for name, reads in (("pairs_of_%d" % a.read_len, lambda: synth_reads(kc, dev, 2 * a.pairs, a.read_len)),
                            ("short_20_to_59", lambda: short_reads(dev, a.seed, a.short_reads & ~1))):
            bases, quals, offs = reads()
            for packed in (False, True):
                out["cases"].append(measure(kc, name + ("_packed" if packed else "_ascii"), bases, quals, offs, packed, a.runs, a.host_reads))
            del bases, quals, offs
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
