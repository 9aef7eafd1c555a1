"""Times kc_trim_adapters on device-resident synthetic pairs (default: 50 M pairs of 2 x 150) and prints one JSON line:
each trim kernel's time (HIP events, best of --runs), the counters, and kc_merge_pairs on the same pairs in the same
run as the yardstick.

The pairs are scripts/merge_pairs_bench.py's (fragments of 200-400 bases: adapter-free, the common case).  With
--short-share S that share of the pairs is rebuilt from a fragment of 60-150 bases: each mate is the fragment (mate 2
reverse-complemented) followed by an adapter of the loaded set, then the bases that were there.
--adapters committed: tests/golden/adapters_no_transposase.fa; synthetic: tests/trim_model.py's 7 500-sequence set."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402
import trim_model as M  # noqa: E402
from merge_pairs_bench import make_pairs  # noqa: E402


def plant_adapters(bases, npairs, mate_len, share, seqs, seed):
    """every round(1 / share)-th pair becomes a short fragment read through into an adapter"""
    dev = bases.device
    step = max(1, round(1 / share))
    rows = torch.arange(0, npairs, step, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n = rows.numel()
    flen = torch.randint(60, 151, (n, 1), generator=g, device=dev)
    amax = max(len(s) for s in seqs)
    table = torch.zeros(len(seqs), amax, dtype=torch.uint8, device=dev)
    alen = torch.tensor([len(s) for s in seqs], device=dev)
    for i, s in enumerate(seqs):
        table[i, :len(s)] = torch.tensor(list(s.encode()), dtype=torch.uint8)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a, c in zip(b"ACGTN", b"TGCAN"):
        comp[a] = c
    v = bases.view(npairs, 2, mate_len)
    pos = torch.arange(mate_len, device=dev).view(1, -1)
    m1 = v[rows, 0]
    frag_rc = comp[torch.gather(m1, 1, (flen - 1 - pos).clamp(min=0)).long()]
    for mate in range(2):
        which = torch.randint(0, len(seqs), (n,), generator=g, device=dev)
        ad = table[which][:, :mate_len] if amax >= mate_len else torch.nn.functional.pad(table[which], (0, mate_len - amax))
        ad_at = torch.gather(ad, 1, (pos - flen).clamp(min=0))
        in_ad = (pos >= flen) & (pos - flen < alen[which].view(-1, 1))
        body = m1 if mate == 0 else frag_rc
        old = v[rows, mate]
        v[rows, mate] = torch.where(pos < flen, body, torch.where(in_ad, ad_at, old))
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--mate-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--adapters", choices=("committed", "synthetic"), default="committed")
    ap.add_argument("--short-share", type=float, default=0.0)
    ap.add_argument("--blastn", action="store_true")
    ap.add_argument("--no-merge", action="store_true", help="skip the kc_merge_pairs yardstick")
    a = ap.parse_args()
    if a.adapters == "committed":
        text = open(os.path.join(ROOT, "tests", "golden", "adapters_no_transposase.fa"), "rb").read()
    else:
        text = M.synthetic_adapters()
    seqs = [l.decode() for l in M.getlines(text) if l[:1] != b">" and len(l) >= 21]
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        counts = kc.load_adapters(text, 21, a.blastn)
        bases, quals, offsets = make_pairs(kc, a.pairs, a.mate_len, a.sub_rate, a.seed)
        planted = plant_adapters(bases, a.pairs, a.mate_len, a.short_share, seqs, a.seed) if a.short_share > 0 else 0
        torch.cuda.synchronize()
        runs = []
        for r in range(a.runs + 1):  # the first call allocates the scratch: not counted
            kc.kernel_times(clear=True)
            t0 = time.perf_counter()
            ob, oq, oo, st = kc.trim_adapters(bases, quals, offsets, paired=True)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            kt = {k: round(v[1], 3) for k, v in kc.kernel_times(clear=True).items() if "trim" in k}
            if r:
                runs.append((wall, kt))
            del ob, oq, oo
        wall, kt = min(runs, key=lambda x: sum(x[1].values()))
        out = dict(metric="trim_adapters", pairs=a.pairs, mate_len=a.mate_len, adapters=a.adapters, adapter_index=counts,
                   blastn=a.blastn, short_share=a.short_share, planted_pairs=planted, kernels_ms=kt,
                   kernel_ms=round(sum(kt.values()), 3), wall_ms=round(wall, 3), stats=st,
                   runs_kernel_ms=[round(sum(x[1].values()), 3) for x in runs])
        if not a.no_merge:
            mruns = []
            for r in range(a.runs + 1):
                kc.kernel_times(clear=True)
                packed, offs, mst = kc.merge_pairs(bases, quals, offsets)
                torch.cuda.synchronize()
                mk = {k: v[1] for k, v in kc.kernel_times(clear=True).items() if k.startswith("kc_merge")}
                if r:
                    mruns.append(sum(mk.values()))
                del packed, offs
            out["merge_pairs_kernel_ms"] = round(min(mruns), 3)
            out["merge_merged"] = mst["merged"]
        print(json.dumps(out))


if __name__ == "__main__":
    main()
