#!/usr/bin/env python3
"""Writes the reference's answers the suite compares against, as data, from oracle/_ref (built by `make -C oracle ref`
where the reference checkout exists):
  * ref_hash_funcs.json  -- MurmurHash3_x64_64 / quick_hash of the reference's src/hash_funcs.c for the inputs of
                            tests/test_oracle_primitives.py::hash_inputs (CPU);
  * ref_gpu_common.npz   -- pack_seq_to_kmer / revcomp / gpu_murmurhash3_64 / comp_nucleotide of the reference's device
                            headers for the inputs of tests/test_gpu_ref_pin.py (needs a GPU).
With the library of a part missing, that part is skipped.  Run from the repo root:
    python tests/golden/make_ref_vectors.py [--out DIR] [--part hash_funcs|gpu_common]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def hash_funcs(out_dir):
    import test_oracle_primitives as T
    if not os.path.exists(T.REF_SO):
        print("skipped ref_hash_funcs.json: %s not built" % T.REF_SO)
        return
    ref = T.ref_hash_lib()
    bufs, words = T.hash_inputs()
    out = {"source": "oracle/_ref/libref_hash_funcs.so = reference src/hash_funcs.c compiled unmodified; "
                     "inputs: tests/test_oracle_primitives.py::hash_inputs",
           "inputs_sha256": T.hash_inputs_sha256(bufs, words),
           "murmur3_x64_64": [hex(ref.MurmurHash3_x64_64(buf.ctypes.data, n)) for n, buf in bufs],
           "quick_hash": [hex(ref.quick_hash(v)) for v in words]}
    path = os.path.join(out_dir, "ref_hash_funcs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


def gpu_common(out_dir):
    import test_gpu_ref_pin as T
    if not os.path.exists(T.REF_SO):
        print("skipped ref_gpu_common.npz: %s not built" % T.REF_SO)
        return
    path = os.path.join(out_dir, "ref_gpu_common.npz")
    np.savez_compressed(path, **T.reference_vectors_live())
    print("wrote", path)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--part", choices=["hash_funcs", "gpu_common"], action="append")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for part in a.part or ["hash_funcs", "gpu_common"]:
        {"hash_funcs": hash_funcs, "gpu_common": gpu_common}[part](a.out)
