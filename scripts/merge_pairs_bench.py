"""Times kc_merge_pairs on device-resident synthetic pairs (default: 50 M pairs of 2 x 150, one GPU's share of a
full-size paired run) and prints one JSON line: each merge kernel's time, the wall time of the call and the GB/s of
input plus output bytes.

Fragments of 200-400 bases (four lengths, mixed) come from kc_synth_reads_device; mate 1 is a fragment's first
--mate-len bases, mate 2 the reverse complement of its last --mate-len bases with the qualities reversed; each mate then
gets independent low-quality substitutions (rate --sub-rate), so that overlaps disagree."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mhm2_kmer_analysis_v2_amd as pkg  # noqa: E402


def make_pairs(kc, npairs, mate_len, sub_rate, seed, frag_lens=(200, 250, 300, 400), chunk=2_000_000):
    dev = "cuda:%d" % kc.device
    bases = torch.empty(2 * npairs * mate_len, dtype=torch.uint8, device=dev)
    quals = torch.empty_like(bases)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a, c in zip(b"ACGTN", b"TGCAN"):
        comp[a] = c
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    done = 0
    while done < npairs:
        n = min(chunk, npairs - done)
        fl = frag_lens[(done // chunk) % len(frag_lens)]
        p = pkg.synth_params(read_len=fl, seed=seed + done)
        fb = torch.empty(n * fl, dtype=torch.uint8, device=dev)
        fq = torch.empty_like(fb)
        fo = torch.empty(n + 1, dtype=torch.int64, device=dev)
        kc.synth_reads_device(fb, fq, fo, n, first_read=done, params=p)
        fb, fq = fb.view(n, fl), fq.view(n, fl)
        m1b, m1q = fb[:, :mate_len], fq[:, :mate_len]
        m2b, m2q = comp[fb[:, fl - mate_len:].flip(1).long()], fq[:, fl - mate_len:].flip(1)
        pb = torch.stack([m1b, m2b], 1).reshape(n, 2, mate_len)
        pq = torch.stack([m1q, m2q], 1).reshape(n, 2, mate_len).clone()
        hit = torch.rand(pb.shape, generator=g, device=dev) < sub_rate
        pb = torch.where(hit, acgt[torch.randint(0, 4, pb.shape, generator=g, device=dev)], pb)
        pq = torch.where(hit, torch.randint(35, 50, pb.shape, generator=g, device=dev).to(torch.uint8), pq)
        at = 2 * done * mate_len
        bases[at:at + 2 * n * mate_len] = pb.reshape(-1)
        quals[at:at + 2 * n * mate_len] = pq.reshape(-1)
        done += n
        del fb, fq, fo, pb, pq, hit
    offsets = torch.arange(0, 2 * npairs + 1, dtype=torch.int64, device=dev) * mate_len
    return bases, quals, offsets


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--mate-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    with pkg.KmerCounter(21, time_kernels=True) as kc:
        bases, quals, offsets = make_pairs(kc, a.pairs, a.mate_len, a.sub_rate, a.seed)
        torch.cuda.synchronize()
        runs = []
        for r in range(a.runs + 1):  # the first call allocates the scratch: not counted
            kc.kernel_times(clear=True)
            t0 = time.perf_counter()
            packed, offs, st = kc.merge_pairs(bases, quals, offsets)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            kt = {k: v[1] for k, v in kc.kernel_times(clear=True).items() if k.startswith("kc_merge")}
            if r:
                runs.append((wall, kt))
            del packed, offs
        wall, kt = min(runs, key=lambda x: sum(x[1].values()))
        kernel_ms = sum(kt.values())
        in_bytes = 2 * bases.numel() + 8 * offsets.numel()
        out_bytes = st["out_bases"] + 8 * (st["out_reads"] + 1)
        print(json.dumps(dict(metric="merge_pairs", pairs=a.pairs, mate_len=a.mate_len, kernels_ms=kt, kernel_ms=round(kernel_ms, 3),
                              wall_ms=round(wall, 3), gbps=round((in_bytes + out_bytes) / kernel_ms / 1e6, 1), in_gb=round(in_bytes / 1e9, 2),
                              out_gb=round(out_bytes / 1e9, 2), stats=st, runs_kernel_ms=[round(sum(x[1].values()), 3) for x in runs])))


if __name__ == "__main__":
    main()
