"""Times kc_seq_kmer_depths and kc_count_spectrum on a table of bench.py's default synthetic reads (k = 21): the depth track of
400 000 reads x 150 bases, of the run's own unitig block and of 4 M sequences of 20 .. 59 bases, and the spectrum of the
table's counts and of an all-equal counts array of the same size.  Prints one JSON line and writes it to
profiles/kmer_depths_<date>.json.

Reported, per input: the kernels' times by kind (HIP events, KC_FLAG_TIME_KERNELS; the median call of --runs after a
warm-up), windows per second of the windows kernel, its share of the call's kernel time, and two yardsticks made in the
same run: kc_lookup on the same windows, cut and packed beforehand (torch, not timed) -- the same probes without the text
work -- and a device-to-device copy that moves the input's bytes and the track's.  The spectrum stands beside a copy of the
counts array.  No ratio is chosen in advance.  KC_LIB names another build of the library (another run length, another number
of probes in flight, another number of LDS copies: -DKC_KTRACK_RUN, -DKC_KTRACK_FLIGHT, -DKC_SPECT_REP); --label says which.
Needs a GPU: there is no fallback."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
from assembly_fasta_bench import timed  # noqa: E402
from depth_insert_bench import copy_ms  # noqa: E402
from mhm2_kmer_analysis_v2_amd.kcount import _DeviceWords  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, L = 21, 150


def window_keys(seqs, offs, k=K):
    """the packed forward k-mers of every window of the sequences (one word: k <= 32), as the depth call defines a window"""
    n = int(seqs.numel())
    code = torch.full((256,), 4, dtype=torch.int64, device=seqs.device)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = code[ch + 32] = i
    codes = code[seqs.long()]
    bad = torch.zeros(n + 1, dtype=torch.int64, device=seqs.device)
    bad[1:] = torch.cumsum((codes == 4).long(), 0)
    pos = torch.arange(max(n - k + 1, 0), device=seqs.device)
    which = torch.searchsorted(offs, pos, right=True)  # the sequence of pos is which - 1 (empty sequences are passed over)
    ok = (bad[pos + k] == bad[pos]) & (pos + k <= offs[which])
    pos = pos[ok]
    del bad, which, ok
    keys = torch.zeros(int(pos.numel()), dtype=torch.int64, device=seqs.device)
    for j in range(k):
        keys |= codes[pos + j] << (62 - 2 * j)
    return keys


def lookup_ms(kc, keys, reps=5):
    """median time of kc_lookup on device-resident queries (events on the counter's stream around the call)"""
    nq = int(keys.numel())
    counts = torch.empty(nq, dtype=torch.int16, device=keys.device)
    torch.cuda.current_stream().synchronize()
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pkg._lib.check(pkg.lib().kc_lookup(kc._h, keys.data_ptr(), nq, 1, counts.data_ptr(), None, None), "kc_lookup")
        e1.record()
        e1.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], int((counts != 0).sum())


def rate(n, ms):
    return round(n / (ms / 1e3)) if ms else None


def measure_depths(kc, name, seqs, offs, runs):
    nbytes, n = int(seqs.numel()), int(offs.numel()) - 1
    out = dict(input=name, seqs=n, bytes=nbytes, calls={})
    stats = None
    for label, kw in (("track", dict(with_records=False)), ("track_and_records", {}), ("fill_mean", dict(fill_mean=True, with_records=False))):
        ms, kt, all_ms, (_, _, stats) = timed(kc, runs, lambda: kc.kmer_depths(seqs, offs, **kw))
        win_ms = kt.get("kc_ktrack_windows_kernel", (0, 0.0))[1] + kt.get("kc_ktrack_windows_kernel<fill>", (0, 0.0))[1]
        out["calls"][label] = dict(call_kernel_ms=round(ms, 4), runs_kernel_ms=all_ms, windows_kernel_ms=round(win_ms, 4),
                                   windows_per_s=rate(stats["windows"], win_ms), bytes_per_s=rate(nbytes, win_ms),
                                   windows_share_of_call=round(win_ms / ms, 3) if ms else None,
                                   kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()})
    out["stats"] = stats
    keys = window_keys(seqs, offs)
    assert int(keys.numel()) == stats["windows"], (int(keys.numel()), stats["windows"])
    lk, found = lookup_ms(kc, keys)
    assert found == stats["present"], (found, stats["present"])
    del keys
    moved = nbytes + 2 * nbytes  # the text read, the track written
    c = copy_ms(moved, seqs.device)
    win_ms = out["calls"]["track"]["windows_kernel_ms"]
    out.update(lookup_same_windows_ms=round(lk, 4), lookup_windows_per_s=rate(stats["windows"], lk),
               windows_kernel_over_lookup=round(win_ms / lk, 3) if lk else None, copy_of_text_and_track_ms=round(c, 4),
               copy_bytes_per_s=rate(moved, c))
    return out


def short_offsets(seed, n):
    rng = np.random.default_rng(seed)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(rng.integers(20, 60, n))
    return offs


def measure_spectrum(kc, name, runs):
    ms, kt, all_ms, (hist, st) = timed(kc, runs, lambda: kc.count_spectrum(on_device=True))
    hist_ms = kt.get("kc_spect_hist_kernel", (0, 0.0))[1]
    n = st["kmers"]
    c = copy_ms(2 * 2 * n, hist.device)
    return dict(counts=name, kmers=n, stats=st, bins_in_use=int((hist != 0).sum()), call_kernel_ms=round(ms, 4), runs_kernel_ms=all_ms,
                hist_kernel_ms=round(hist_ms, 4), stats_kernel_ms=round(kt.get("kc_spect_stats_kernel", (0, 0.0))[1], 4),
                counts_per_s=rate(n, hist_ms), copy_of_the_counts_ms=round(c, 4), hist_kernel_over_copy=round(hist_ms / c, 3) if c else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=10_000_000, help="reads of bench.py's synthetic stream behind the table")
    ap.add_argument("--query-reads", type=int, default=400_000)
    ap.add_argument("--short-seqs", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--label", default="as built")
    ap.add_argument("--only", default="", help="comma list of reads,unitigs,short,spectrum (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmer_depths_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("kmer_depths_bench.py needs a GPU: the HIP path is the only path")
    only = set(a.only.split(",")) if a.only else {"reads", "unitigs", "short", "spectrum"}
    params = pkg.synth_params()
    est_unique = int(64 * 4_000_000 + a.reads * L * params.sub_error_rate * K * 1.05) + (1 << 20)
    out = dict(metric="kmer_depths", label=a.label, lib=os.path.basename(pkg.lib_path()), k=K, table_reads=a.reads, runs=a.runs, inputs=[], spectrum=[])
    with pkg.KmerCounter(K, max_elems=est_unique, time_kernels=True, max_kmers_buffered=int(a.reads * (L - K - 1) * 1.02) + (1 << 20)) as kc:
        dev = "cuda:%d" % kc.device
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(stream)
        kc.set_stream(stream.cuda_stream)
        d_bases = torch.empty(a.reads * L, dtype=torch.uint8, device=dev)
        d_quals = torch.empty(a.reads * L, dtype=torch.uint8, device=dev)
        d_offs = torch.empty(a.reads + 1, dtype=torch.int64, device=dev)
        kc.synth_reads_device(d_bases, d_quals, d_offs, a.reads, params=params)
        torch.cuda.synchronize()
        kc.submit_reads(d_bases, d_quals, d_offs)
        res = kc.finalize()
        del d_quals
        out["results"] = int(res.n)
        if "reads" in only:
            nq = min(a.query_reads, a.reads)
            out["inputs"].append(measure_depths(kc, "reads_%dx%d" % (nq, L), d_bases[:nq * L], d_offs[:nq + 1].clone(), a.runs))
        if "short" in only:
            offs = short_offsets(a.seed, a.short_seqs)
            need = int(offs[-1])
            assert need <= int(d_bases.numel())
            out["inputs"].append(measure_depths(kc, "short_%d_of_20_to_59" % a.short_seqs, d_bases[:need], torch.from_numpy(offs).to(dev), a.runs))
        if "spectrum" in only:
            out["spectrum"].append(measure_spectrum(kc, "the table's", a.runs))
            res = kc.finalize()
            words = _DeviceWords(res.d_counts, int(res.n) * 2 // 8, dev).tensor()
            saved = words.clone()
            words.fill_(0x0005000500050005)
            torch.cuda.current_stream().synchronize()
            out["spectrum"].append(measure_spectrum(kc, "all equal (5)", a.runs))
            words.copy_(saved)
            torch.cuda.current_stream().synchronize()
            del saved, words
        if "unitigs" in only:  # last: it sorts the results
            del d_bases
            seqs, offsets, _, ust = kc.unitigs()
            b = measure_depths(kc, "unitig_block", seqs, offsets, a.runs)
            b["unitig_stats"] = ust
            out["inputs"].append(b)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.label != "as built" else "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
