"""Regenerates tests/golden/gap_ref_alignments.json: what the reference's own aligner answers for the seeded read-sized
cases of tests/gap_model.py::gap_ssw_cases, in all five fields of Aligner::Align(report_cigar = false).

Needs the reference checkout (MHM2_REFERENCE, default /root/reference).  Its src/ssw/ssw.cpp and ssw_core.cpp are
compiled unmodified with g++, together with the small driver below, into a temporary directory outside the tree.  Only
the recorded numbers are written here, and a SHA-256 of the inputs; the test regenerates the inputs from the seed.  The
script then checks tests/trim_model.py's aligner against every case and fails if one differs.

    python tests/golden/make_gap_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gap_model as G  # noqa: E402
import trim_model as M  # noqa: E402

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include "ssw.hpp"
int main(int argc, char **argv) {
  StripedSmithWaterman::Aligner aligner;
  aligner.Clear();
  if (!aligner.ReBuild(std::string(argv[1]))) return 2;
  StripedSmithWaterman::Filter filter;
  filter.report_cigar = false;
  std::string q, r;
  while (std::cin >> q >> r) {
    StripedSmithWaterman::Alignment a;
    aligner.Align(q.data(), (int)q.length(), r.data(), (int)r.length(), filter, &a, std::max((int)(r.length() / 2), 15));
    printf("%d %d %d %d %d\n", (int)a.sw_score, (int)a.ref_begin, (int)a.ref_end, (int)a.query_begin, (int)a.query_end);
  }
  return 0;
}
"""
FIELDS = ("sw_score", "ref_begin", "ref_end", "query_begin", "query_end")
SETS = ("11111", "23521", "13521")


def inputs_sha256(cases):
    h = hashlib.sha256()
    for q, r in cases:
        h.update(q.encode() + b" " + r.encode() + b"\n")
    return h.hexdigest()


def main():
    ref = os.environ.get("MHM2_REFERENCE", "/root/reference")
    ssw = os.path.join(ref, "src", "ssw")
    if not os.path.exists(os.path.join(ssw, "ssw_core.cpp")):
        sys.exit("no reference checkout at %s" % ref)
    out = {"source": "reference src/ssw/ssw.cpp + ssw_core.cpp compiled unmodified (g++ -O2) with the driver of "
                     "tests/golden/make_gap_golden.py; inputs: tests/gap_model.py::gap_ssw_cases",
           "fields": list(FIELDS), "sets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cpp")
        open(drv, "w").write(DRIVER)
        exe = os.path.join(tmp, "ssw_driver")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", ssw, "-o", exe, drv, os.path.join(ssw, "ssw.cpp"),
                               os.path.join(ssw, "ssw_core.cpp")])
        for name in SETS:
            cases = G.gap_ssw_cases(name)
            assert all(q and r and " " not in q + r for q, r in cases)
            text = "".join("%s %s\n" % c for c in cases)
            res = subprocess.run([exe, name], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
            rows = [[int(x) for x in l.split()] for l in res if l]
            assert len(rows) == len(cases), (len(rows), len(cases))
            out["sets"][name] = {"n": len(cases), "inputs_sha256": inputs_sha256(cases),
                                 "results": " ".join(",".join(str(v) for v in row) for row in rows)}
            scores = G.SCORE_SETS[name]
            bad = 0
            for (q, r), row in zip(cases, rows):
                got = M.ssw_align(q.encode(), r.encode(), scores)
                if [got[f] for f in FIELDS] != row:
                    bad += 1
                    if bad <= 10:
                        print("MISMATCH", name, q, r, row, [got[f] for f in FIELDS])
            hi = sum(1 for row in rows if row[0] + max(scores[1], scores[4]) >= 255)
            print("%s: %d cases, %d differ from the model, %d reach the word lanes" % (name, len(cases), bad, hi))
            if bad:
                sys.exit(1)
    with open(os.path.join(HERE, "gap_ref_alignments.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
