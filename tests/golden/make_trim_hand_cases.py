"""Regenerates tests/golden/trim_hand_cases.json: hand-built reads around the corners of Adapters::trim / trim_pair, with
what tests/trim_model.py answers for them (the GPU test compares the library with the model and with this record).

    python tests/golden/make_trim_hand_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import trim_model as M  # noqa: E402

A = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"          # 34 bases
B = "CTGTCTCTTATACACATCTCCGAGCCCACGAGAC"          # 34 bases
INS = "TTGACCATGCATTGCAAGGCTTACGGATCCATGCAAGTTCAGGCTAACCGTTAGC"  # 55 bases, shares no k-mer with A or B
FILL = "CATGCATGGTTGACCAGGTTAACCAGTCGATCAGCTAGCTAGGATCGATCCGGATTA"
TWO = (">A\n%s\n>B\n%s\n" % (A, B))


def comp(s):  # a base that differs at every position
    return s.translate(str.maketrans("ACGT", "CATG"))


CASES = []


def case(name, reads, k=21, blastn=False, paired=False, adapters=TWO):
    CASES.append(dict(name=name, adapters=adapters, k=k, blastn=blastn, paired=paired, reads=reads))


for cut in (11, 12, 13):
    case("cut at %d" % cut, [INS[:cut] + A, INS[:cut] + A + FILL[:9]])
# identity = score / 34: 16, 17 (exactly 0.5) and 18 bases of A, then Ns, which score against everything; k = 15 seeds them
for n in (16, 17, 18):
    case("identity %d/34" % n, [INS[:40] + A[:n] + "N" * 30], k=15)
    case("identity %d/34 blastn" % n, [INS[:40] + A[:n] + "N" * 30], k=15, blastn=True)
# 33/34 > 0.97 ends the scan, so B behind it is never aligned; 32/34 does not
for sc in (False, True):
    case("identity 33/34 ends the scan%s" % (" blastn" if sc else ""), [INS[:40] + A[:33] + "NNN" + B], blastn=sc)
    case("identity 32/34 goes on%s" % (" blastn" if sc else ""), [INS[:40] + A[:32] + "NNNN" + B], blastn=sc)
case("identity 34/34 then B", [INS[:40] + A + B])
case("shorter than k", [A[:20], A[:21], "", "A", INS[:20]])
case("two adapters in one read", [INS[:30] + B[:28] + FILL[:10] + A, INS[:30] + A[:25] + FILL[:13] + B])
case("the same adapter twice", [INS[:24] + A + FILL[:20] + A, INS[:16] + A[:26] + FILL[:30] + A[:30]])
case("reverse strand", [INS[:33] + M.revcomp(A.encode()).decode(), INS[:20] + M.revcomp(B.encode()).decode()[:30]])
case("lower case, N and IUPAC in the read", [INS[:36].lower() + A[:10] + "N" + A[11:], INS[:36] + A[:12] + "R" + A[13:].lower()])
# trim_pair: a mate left at length 0, 1 and 2; an untrimmed mate shortened by its partner
case("pair: partner at 0", [INS[:5] + A, INS], paired=True)
case("pair: untrimmed mate of length 1", ["G", INS[:30] + A], paired=True)
case("pair: untrimmed mate of length 2", ["GT", INS[:30] + A], paired=True)
case("pair: untrimmed mate shortened", [INS + FILL, INS[:30] + A], paired=True)
case("pair: both trimmed, different lengths", [INS[:44] + A, INS[:30] + B], paired=True)
case("pair: a short match below one half", [INS[:40] + FILL[:20], INS[:28] + A[:16] + "N" * 20], k=15, paired=True)
case("pair: neither trimmed", [INS, FILL, INS[:10], ""], paired=True)
case("unpaired twins of the pair cases", [INS[:5] + A, INS, "G", INS[:30] + A, INS + FILL, INS[:30] + A])
case("poly-G read against an N adapter", ["G" * 60, INS[:20] + "G" * 30], adapters=">n\n%s\n" % ("N" * 30))
case("empty adapter set", [INS + A, A], adapters=">short\nACGT\n")


def quals_of(c, r, n):
    return "".join(chr(35 + (7 * c + 3 * r + j) % 40) for j in range(n))


def main():
    out = []
    for ci, c in enumerate(CASES):
        ads = M.AdapterSet(c["adapters"].encode(), c["k"], c["blastn"])
        bases = "".join(c["reads"]).encode()
        quals = "".join(quals_of(ci, r, len(s)) for r, s in enumerate(c["reads"])).encode()
        offs = [0]
        for s in c["reads"]:
            offs.append(offs[-1] + len(s))
        _, _, oo, st = M.trim_reads(ads, list(bases), list(quals), offs, c["paired"])
        c = dict(c, quals=quals.decode(), expect_lens=[int(oo[i + 1] - oo[i]) for i in range(len(c["reads"]))], expect_stats=st)
        out.append(c)
        print("%-45s lens %s -> %s  %s" % (c["name"], [len(s) for s in c["reads"]], c["expect_lens"], st))
    with open(os.path.join(HERE, "trim_hand_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
