"""Times the device FASTQ parsers (kc_fastq_to_packed_device, kc_fastq_pairs_device) on device-resident FASTQ text and
prints one JSON line: per-kernel HIP-event times, GB/s of text, the host parser on the 1 M-read text (its time at the
larger size is extrapolated and labelled so), and, apart, a fresh counter's creation and the time from FASTQ text on the
device to kc_finalize.  The unpaired text is also timed at a base 5 bytes above a 16-byte boundary (--misalign).

The reads are kc_synth_reads_device's (150 bases, --reads of them); each record gets an Illumina-style name of realistic
length with the read number in it.  "pairs" is the same text as two files of --reads records each (mate 2 = the next
read number), so its text is twice as long."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from mhm2_kmer_analysis_v2_amd import _lib  # noqa: E402

NAME = b"@A00123:456:HJKLMNDXX:1:1101:%010d:1000 1:N:0:ACGTACGT+TGCATGCA"


def make_text(kc, nreads, first, read_len=150, chunk=4_000_000, seed=1):
    """FASTQ text of nreads synthetic reads on the device"""
    dev = "cuda:%d" % kc.device
    nl = len(NAME % 0)
    rec = nl + 1 + read_len + 3 + read_len + 1
    text = torch.empty(nreads * rec, dtype=torch.uint8, device=dev)
    tv = text.view(nreads, rec)
    tmpl = torch.frombuffer(bytearray(NAME % 0 + b"\n" + b"A" * read_len + b"\n+\n" + b"I" * read_len + b"\n"), dtype=torch.uint8).to(dev)
    tv[:] = tmpl
    p = pkg.synth_params(read_len=read_len, seed=seed)
    pw = torch.tensor([10 ** (9 - i) for i in range(10)], dtype=torch.int64, device=dev)
    d0 = nl - len(b"%010d:1000 1:N:0:ACGTACGT+TGCATGCA" % 0)  # first digit of the read number
    for at in range(0, nreads, chunk):
        n = min(chunk, nreads - at)
        b = torch.empty(n * read_len, dtype=torch.uint8, device=dev)
        q = torch.empty_like(b)
        o = torch.empty(n + 1, dtype=torch.int64, device=dev)
        kc.synth_reads_device(b, q, o, n, first_read=first + at, params=p)
        tv[at:at + n, nl + 1:nl + 1 + read_len] = b.view(n, read_len)
        tv[at:at + n, nl + 4 + read_len:nl + 4 + 2 * read_len] = q.view(n, read_len)
        num = torch.arange(first + at, first + at + n, dtype=torch.int64, device=dev)
        tv[at:at + n, d0:d0 + 10] = ((num[:, None] // pw[None, :]) % 10 + 48).to(torch.uint8)
        del b, q, o
    return text, rec


def parse(kc, texts, nreads, read_len, pairs):
    L = pkg.lib()
    dev = "cuda:%d" % kc.device
    nr, nb, c1, c2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    nout = nreads * (2 if pairs else 1)
    offs = torch.empty(nout + 1, dtype=torch.int64, device=dev)
    if pairs:
        bases = torch.empty(nout * read_len, dtype=torch.uint8, device=dev)
        quals = torch.empty_like(bases)
        st = L.kc_fastq_pairs_device(kc._h, texts[0].data_ptr(), texts[0].numel(), texts[1].data_ptr(), texts[1].numel(), 1, 0,
                                     bases.data_ptr(), quals.data_ptr(), bases.numel(), offs.data_ptr(), nout, C.byref(nr), C.byref(nb),
                                     C.byref(c1), C.byref(c2))
        out = (bases, quals, offs)
    else:
        packed = torch.empty(nout * read_len, dtype=torch.uint8, device=dev)
        st = L.kc_fastq_to_packed_device(kc._h, texts[0].data_ptr(), texts[0].numel(), 1, 0, packed.data_ptr(), packed.numel(),
                                         offs.data_ptr(), nout, C.byref(nr), C.byref(nb), C.byref(c1))
        out = (packed, offs)
    _lib.check(st, "fastq parse")
    assert nr.value == nout and nb.value == nout * read_len
    return out


def time_parse(kc, texts, nreads, read_len, pairs, runs):
    best = None
    for r in range(runs + 1):  # the first call allocates the scratch: not counted
        kc.kernel_times(clear=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parse(kc, texts, nreads, read_len, pairs)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        kt = {k: v[1] for k, v in kc.kernel_times(clear=True).items() if k.startswith("kc_fq")}
        del out
        if r and (best is None or sum(kt.values()) < sum(best[1].values())):
            best = (wall, kt)
    wall, kt = best
    text_bytes = sum(t.numel() for t in texts)
    ms = sum(kt.values())
    return dict(text_gb=round(text_bytes / 1e9, 3), kernels_ms=kt, kernel_ms=round(ms, 3), wall_ms=round(wall, 3),
                text_gbps=round(text_bytes / ms / 1e6, 1))


def host_parse_ms(texts, pairs):
    h = [t.cpu().numpy().tobytes() for t in texts]
    t0 = time.perf_counter()
    if pairs:
        pkg.fastq_pairs(h[0], h[1])
    else:
        pkg.fastq_to_packed(h[0])
    return (time.perf_counter() - t0) * 1e3


def end_to_end_ms(k, text, nreads, read_len):
    """(counter creation, FASTQ text on the device -> kc_finalize) in ms, one fresh counter sized for the input the way
    bench.py sizes its own (distinct k-mers: the synthetic genomes plus about k per substitution error; every k-mer
    occurrence buffered, so the count runs in one pass)"""
    params = pkg.synth_params()
    est_unique = int(64 * 4_000_000 + nreads * read_len * params.sub_error_rate * k * 1.05) + (1 << 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pkg.KmerCounter(k, max_elems=est_unique, max_kmers_buffered=int(nreads * (read_len - k - 1) * 1.02) + (1 << 20),
                         wire_units=True) as kc:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        packed, offs = parse(kc, [text], nreads, read_len, False)
        kc.submit_packed_reads(packed, offs, nreads=nreads)
        del packed, offs
        kc.finalize()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def misaligned(text, shift):
    """the same text at `shift` bytes above a 16-byte boundary (the base a streamed block gets)"""
    buf = torch.empty(text.numel() + 16, dtype=torch.uint8, device=text.device)
    view = buf[shift:shift + text.numel()]
    view.copy_(text)
    return buf, view


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--host-reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--skip-pairs", action="store_true")
    ap.add_argument("--skip-host", action="store_true", help="no host-parser timing (counter collection runs)")
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--misalign", type=int, default=5, help="also time the unpaired text at this many bytes above a 16-byte "
                    "boundary (0: no)")
    a = ap.parse_args()
    res = dict(metric="fastq_parse", reads=a.reads, read_len=a.read_len, name_len=len(NAME % 0))
    with pkg.KmerCounter(a.k, time_kernels=True) as kc:
        for n in sorted({a.host_reads, a.reads}):
            key = "%dM" % (n // 1_000_000) if n >= 1_000_000 else str(n)
            t1, rec = make_text(kc, n, 0, a.read_len)
            torch.cuda.synchronize()
            r = dict(unpaired=time_parse(kc, [t1], n, a.read_len, False, a.runs), record_bytes=rec)
            if a.misalign:
                buf, view = misaligned(t1, a.misalign)
                assert view.data_ptr() % 16 == a.misalign % 16
                r["unpaired_base_misaligned_by_%d" % a.misalign] = time_parse(kc, [view], n, a.read_len, False, a.runs)
                del buf, view
            if n == a.host_reads and not a.skip_host:
                r["host_unpaired_ms"] = round(host_parse_ms([t1], False), 1)
            if not a.skip_pairs:
                t2, _ = make_text(kc, n, n, a.read_len)
                r["pairs"] = time_parse(kc, [t1, t2], n, a.read_len, True, a.runs)
                if n == a.host_reads and not a.skip_host:
                    r["host_pairs_ms"] = round(host_parse_ms([t1, t2], True), 1)
                del t2
            if n == a.reads and not a.skip_end_to_end:
                create, run = end_to_end_ms(a.k, t1, n, a.read_len)
                r["counter_creation_k%d_ms" % a.k] = round(create, 1)
                r["parse_submit_finalize_k%d_ms" % a.k] = round(run, 1)
            del t1
            torch.cuda.empty_cache()
            res[key] = r
    h = res.get("%dM" % (a.host_reads // 1_000_000), {})
    scale = a.reads / a.host_reads
    if "host_unpaired_ms" in h:
        res["host_unpaired_ms_extrapolated_to_%d_reads" % a.reads] = round(h["host_unpaired_ms"] * scale, 1)
    if "host_pairs_ms" in h:
        res["host_pairs_ms_extrapolated_to_%d_reads" % a.reads] = round(h["host_pairs_ms"] * scale, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
