"""Times kc_correct_reads on a table of bench.py's default synthetic reads (k = 21): 400 000 error-free reads x 150 bases of the
same genomes with substitutions planted at 0.5 %, and 4 M sequences of 20 .. 59 bases cut from them.  Prints one JSON line and
writes it to profiles/correct_reads_<date>.json.

Reported, per input: the kernels' times by kind (HIP events, KC_FLAG_TIME_KERNELS; the median call of --runs after a warm-up)
of a call of one, two and three rounds -- the difference of two calls is what the later round costs -- and the yardstick made
in the same run: kc_seq_kmer_depths' track pass on the same reads.  The call cannot cost less than its track passes, so it is
given as a multiple of one.  The evaluation kernel's sites per second, and its probes per second as an upper bound (3 k probes a
site; a range shorter than k, or an alternative whose first window is not solid, asks fewer).  Of the planted errors, the share
that out holds corrected; the false corrections: bytes of out that differ from the error-free read and were not planted, or were
planted and became a third base.  No ratio is chosen in advance.  Needs a GPU: there is no fallback."""
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
from kmer_depths_bench import rate, short_offsets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, L = 21, 150
EVAL, TRACK = "kc_correct_eval_kernel", "kc_ktrack_windows_kernel<correct>"


def plant(clean, rate_, seed):
    """the text with a wrong base at `rate_` of its bases (upper-case A C G T only), and where"""
    g = torch.Generator(device=clean.device)
    g.manual_seed(seed)
    code = torch.full((256,), 4, dtype=torch.int64, device=clean.device)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    codes = code[clean.long()]
    where = (torch.rand(clean.numel(), generator=g, device=clean.device) < rate_) & (codes < 4)
    shift = torch.randint(1, 4, (clean.numel(),), generator=g, device=clean.device)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=clean.device)
    noisy = torch.where(where, letters[(codes + shift) % 4], clean)
    return noisy, where


def measure(kc, name, clean, noisy, planted, offs, runs):
    nbytes, n = int(clean.numel()), int(offs.numel()) - 1
    out = dict(input=name, seqs=n, bytes=nbytes, planted=int(planted.sum()), calls={})
    ms, kt, all_ms, (_, _, dst) = timed(kc, runs, lambda: kc.kmer_depths(noisy, offs, min_count=2, with_records=False))
    track_ms = kt["kc_ktrack_windows_kernel"][1]
    out.update(track_pass_ms=round(track_ms, 4), track_windows_per_s=rate(dst["windows"], track_ms), depth_stats=dst)
    for rounds in (1, 2, 3):
        ms, kt, all_ms, (fixed, _, _, st) = timed(kc, runs, lambda: kc.correct_reads(noisy, offs, rounds=rounds, with_records=True))
        ev = kt.get(EVAL, (0, 0.0))[1]
        healed = int(((fixed == clean) & planted).sum())
        false_ = int(((fixed != clean) & ~planted).sum()) + int(((fixed != clean) & (fixed != noisy) & planted).sum())
        out["calls"]["rounds_%d" % rounds] = dict(
            call_kernel_ms=round(ms, 4), runs_kernel_ms=all_ms, over_one_track_pass=round(ms / track_ms, 3), track_passes=kt[TRACK][0],
            track_share_of_call=round(kt[TRACK][1] / ms, 3), eval_kernel_ms=round(ev, 4), sites_per_s=rate(st["sites"], ev),
            probes_per_s_at_most=rate(st["sites"] * 3 * K, ev), stats=st, planted_recovered=healed,
            recovered_share=round(healed / max(int(planted.sum()), 1), 4), false_corrections=false_,
            kernels={k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in kt.items()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=10_000_000, help="reads of bench.py's synthetic stream behind the table")
    ap.add_argument("--query-reads", type=int, default=400_000)
    ap.add_argument("--short-seqs", type=int, default=4_000_000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_reads_%s.json" % datetime.date.today().isoformat()))
    a = ap.parse_args()
    if not torch.cuda.is_available() or pkg.lib().kc_device_count() < 1:
        raise SystemExit("correct_reads_bench.py needs a GPU: the HIP path is the only path")
    params = pkg.synth_params()
    est_unique = int(64 * 4_000_000 + a.reads * L * params.sub_error_rate * K * 1.05) + (1 << 20)
    out = dict(metric="correct_reads", lib=os.path.basename(pkg.lib_path()), k=K, table_reads=a.reads, runs=a.runs, error_rate=a.error_rate, inputs=[])
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
        out["results"] = int(kc.finalize().n)
        # the same genomes read without errors: what the planted reads are judged against
        nq = max(a.query_reads, (a.short_seqs * 60 + L - 1) // L)
        clean_params = pkg.synth_params(sub_error_rate=0.0, n_rate=0.0, lowq_rate=0.0)
        kc.synth_reads_device(d_bases[:nq * L], d_quals[:nq * L], d_offs[:nq + 1], nq, params=clean_params)
        torch.cuda.synchronize()
        clean = d_bases[:nq * L].clone()
        del d_bases, d_quals
        noisy, planted = plant(clean, a.error_rate, a.seed)
        nb = a.query_reads * L
        out["inputs"].append(measure(kc, "reads_%dx%d" % (a.query_reads, L), clean[:nb], noisy[:nb], planted[:nb], d_offs[:a.query_reads + 1].clone(), a.runs))
        offs = short_offsets(a.seed, a.short_seqs)
        nb = int(offs[-1])
        out["inputs"].append(measure(kc, "short_%d_of_20_to_59" % a.short_seqs, clean[:nb], noisy[:nb], planted[:nb], torch.from_numpy(offs).to(dev), a.runs))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(line + "\n")


if __name__ == "__main__":
    main()
