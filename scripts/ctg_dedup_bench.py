"""Times kc_ctg_dedup on three blocks: the 40 000-contig block scripts/scaffold_bench.py builds with a tenth as many planted
contained copies (many short candidates), the heavy-tailed block of scripts/assembly_fasta_bench.py with its longest contig
duplicated (few very long ones), 4 M contigs of 20 .. 59 bases, and single duplicate pairs at and beyond the length at which
a candidate is cut into segments.  Prints one JSON line and writes it to profiles/ctg_dedup_<date>.json.

Reported, per block: the kernels' times by kind (HIP events, KC_FLAG_TIME_KERNELS; the median call of --runs after a
warm-up), the windows passes as block bytes per second, the verify pass as compared bytes per second (both sides of every
candidate, read once each) and the gathers as output bytes per second -- the last two beside a device-to-device copy that
moves the same number of bytes, made in the same run: that copy is the yardstick, no ratio chosen in advance.  The compared
bytes are counted from the records: both sides of every removed contig, once, which is what the verify pass reads at least.
Needs a GPU: there is no fallback."""
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
from assembly_fasta_bench import heavy_block, scaffold_bench_block, timed  # noqa: E402
from depth_insert_bench import copy_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def with_contained_copies(seqs, offs, rng, share=0.1, k=21):
    """the block with share * contigs slices of its contigs appended, every other one flipped"""
    text, o = seqs.cpu().numpy().tobytes(), offs.cpu().numpy()
    n = len(o) - 1
    extra = []
    for u in rng.integers(0, n, int(n * share)):
        t = text[int(o[u]):int(o[u + 1]) - 1]
        if len(t) <= k + 1:
            continue
        a = int(rng.integers(0, len(t) - k))
        t = t[a:a + int(rng.integers(k, len(t) - a + 1))]
        extra.append(t.translate(COMP)[::-1] if len(extra) & 1 else t)
    block = text + b"".join(t + b"_" for t in extra)
    offsets = np.concatenate([o[:-1], int(o[-1]) + np.concatenate([[0], np.cumsum([len(t) + 1 for t in extra])])]).astype(np.int64)
    dev = seqs.device
    return torch.from_numpy(np.frombuffer(block, dtype=np.uint8).copy()).to(dev), torch.from_numpy(offsets).to(dev), len(extra)


def with_longest_duplicated(seqs, offs):
    lens = offs[1:] - offs[:-1]
    u = int(torch.argmax(lens))
    copy = seqs[int(offs[u]):int(offs[u + 1])]
    return torch.cat([seqs, copy]), torch.cat([offs, offs[-1:] + copy.numel()]), int(copy.numel()) - 1


def tiny_block(dev, seed, n):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(20, 60, n).astype(np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths + 1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    seqs = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (int(offs[-1]),), generator=gen, device=dev)]
    d_offs = torch.from_numpy(offs).to(dev)
    seqs[d_offs[1:] - 1] = ord("_")
    return seqs, d_offs


def pair_block(dev, seed, n):
    """two equal contigs of n random bases: one candidate, one wave up to 16 384 bases, a wave every 8 192 beyond"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    t = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n + 1,), generator=gen, device=dev)]
    t[n] = ord("_")
    return torch.cat([t, t]), torch.tensor([0, n + 1, 2 * n + 2], dtype=torch.int64, device=dev)


def rate(nbytes, ms):
    return round(nbytes / (ms / 1e3)) if ms else None


def measure(kc, name, seqs, offs, runs, with_depths, **kw):
    dev = seqs.device
    nbytes, n = int(seqs.numel()), int(offs.numel()) - 1
    depths = torch.ones(nbytes, dtype=torch.int16, device=dev) if with_depths else None
    ms, kt, all_ms, res = timed(kc, runs, lambda: kc.dedup_contigs(seqs, offs, depths, **kw))
    out_seqs, _, _, recs, st = res
    one = lambda k: kt.get(k, (0, 0.0))[1]  # noqa: E731
    r = recs.cpu().numpy().view(pkg.kcount.DEDUP_DTYPE)
    # what the verify pass reads: both sides of every candidate; the candidates are not handed out, so the removed contigs'
    # bytes (each verified at least once) are the floor that is reported, beside the pass's time
    removed = int(r["len"][r["status"] != 0].sum())
    windows_ms = one("kc_dedup_windows_kernel<count>") + one("kc_dedup_windows_kernel<write>")
    verify_ms = one("kc_dedup_verify_kernel") + one("kc_dedup_verify_kernel<long>")
    gather_ms, out_bytes = one("kc_dedup_gather_kernel"), int(out_seqs.numel())
    out = dict(block=name, contigs=n, block_bytes=nbytes, params=kw, stats=st, call_kernel_ms=round(ms, 3), runs_kernel_ms=all_ms,
               kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()},
               windows_two_passes_ms=round(windows_ms, 4), windows_block_bytes_per_s=rate(2 * nbytes, windows_ms),
               verify_ms=round(verify_ms, 4), verify_compared_bytes=2 * removed, verify_compared_bytes_per_s=rate(2 * removed, verify_ms),
               gather_ms=round(gather_ms, 4), gather_output_bytes=out_bytes, gather_output_bytes_per_s=rate(out_bytes, gather_ms))
    if verify_ms and removed:
        c = copy_ms(2 * removed, dev)
        out.update(copy_of_the_compared_bytes_ms=round(c, 4), verify_share_of_copy_rate=round(c / verify_ms, 3))
    if gather_ms:
        c = copy_ms(2 * out_bytes, dev)
        out.update(copy_of_the_output_ms=round(c, 4), gather_share_of_copy_rate=round(c / gather_ms, 3))
        if with_depths:
            d_ms = one("kc_dedup_gather_kernel<depths>")
            c = copy_ms(4 * out_bytes, dev)
            out.update(gather_depths_ms=round(d_ms, 4), copy_of_the_depths_ms=round(c, 4), gather_depths_share_of_copy_rate=round(c / d_ms, 3))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--heavy-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--tiny-contigs", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctg_dedup_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("ctg_dedup_bench.py needs a GPU: the HIP path is the only path")
    out = dict(metric="ctg_dedup", seed=a.seed, runs=a.runs, blocks=[])
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        dev = "cuda:%d" % kc.device
        t0 = time.perf_counter()
        seqs, offs, planted = with_contained_copies(*scaffold_bench_block(dev), np.random.default_rng(a.seed))
        out["host_input_s"] = round(time.perf_counter() - t0, 1)
        b = measure(kc, "scaffold_bench_with_copies", seqs, offs, a.runs, True)
        b["planted"] = planted
        if b["stats"]["contained"] + b["stats"]["duplicates"] < planted:
            raise SystemExit("scaffold_bench_with_copies: %d planted copies, %d removed" % (planted, b["stats"]["contained"] + b["stats"]["duplicates"]))
        out["blocks"].append(b)
        del seqs, offs
        seqs, offs, longest = with_longest_duplicated(*heavy_block(dev, a.seed, a.heavy_bytes))
        b = measure(kc, "heavy_tailed_longest_duplicated", seqs, offs, a.runs, False)
        b["longest"] = longest
        if b["stats"]["duplicates"] < 1 or b["stats"]["longest_removed"] != longest:
            raise SystemExit("heavy_tailed_longest_duplicated: the copy of the longest contig was not removed")
        out["blocks"].append(b)
        del seqs, offs
        seqs, offs = tiny_block(dev, a.seed, a.tiny_contigs)
        out["blocks"].append(measure(kc, "tiny_contigs", seqs, offs, a.runs, True))
        del seqs, offs
        # where the cut lies: the same pair as one wave and, a base longer, as three segments; then longer pairs
        for n in (16384, 16385, 262144, 4194304):
            out["blocks"].append(measure(kc, "pair_of_%d" % n, *pair_block(dev, a.seed, n), a.runs, False))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
