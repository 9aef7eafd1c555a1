"""Hand cases of kc_ctg_dedup, shared by tests/test_dedup_model.py (the model holds them) and tests/test_gpu_ctg_dedup.py
(the device equals the model on them).  cases(k) -> [(name, contigs, keywords of the call, want)]: want maps every
REMOVED contig to (status, container, pos, orient, mismatches); every other contig is kept."""
import random

from dedup_model import CONTAINED, DUPLICATE, rc

KS = (21, 32, 33, 55, 77, 99)  # every NL = 1 .. 4, and one even k


def rnd(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"ACGT") for _ in range(n))


def cases(k):
    out = []

    def case(name, ctgs, want, **kw):
        out.append((name, [bytes(c) for c in ctgs], kw, want))

    a = rnd(3 * k + 7, 1)
    case("duplicates, same strand", [a, a], {1: (DUPLICATE, 0, 0, 0, 0)})
    case("duplicates, opposite strand", [a, rc(a)], {1: (DUPLICATE, 0, 0, 1, 0)})
    case("three equal copies", [a, a, a], {1: (DUPLICATE, 0, 0, 0, 0), 2: (DUPLICATE, 0, 0, 0, 0)})
    case("three equal copies, the middle one flipped", [a, rc(a), a], {1: (DUPLICATE, 0, 0, 1, 0), 2: (DUPLICATE, 0, 0, 0, 0)})
    # containment at the container's first byte, its last byte and inside it, on both strands; six different lengths
    b = rnd(6 * k + 41, 2)
    n = len(b)
    m = [k, k + 1, k + 17, 2 * k + 3, 2 * k + 16, 3 * k]
    parts = [b[:m[0]], b[n - m[1]:], b[5:5 + m[2]], rc(b[:m[3]]), rc(b[n - m[4]:]), rc(b[7:7 + m[5]])]
    case("contained at the first byte, the last byte and inside, both strands", [b] + parts,
         {1: (CONTAINED, 0, 0, 0, 0), 2: (CONTAINED, 0, n - m[1], 0, 0), 3: (CONTAINED, 0, 5, 0, 0), 4: (CONTAINED, 0, 0, 1, 0),
          5: (CONTAINED, 0, n - m[4], 1, 0), 6: (CONTAINED, 0, 7, 1, 0)})
    case("the same, the container last", parts + [b],
         {0: (CONTAINED, 6, 0, 0, 0), 1: (CONTAINED, 6, n - m[1], 0, 0), 2: (CONTAINED, 6, 5, 0, 0), 3: (CONTAINED, 6, 0, 1, 0),
          4: (CONTAINED, 6, n - m[4], 1, 0), 5: (CONTAINED, 6, 7, 1, 0)})
    # a chain u in v in w: both records name w
    w = rnd(5 * k + 30, 3)
    v = w[3:3 + 2 * k + 20]
    u = v[2:2 + k + 5]
    case("a chain: both name the longest", [u, v, w], {0: (CONTAINED, 2, 5, 0, 0), 1: (CONTAINED, 2, 3, 0, 0)})
    # a contig that is its own reverse complement: alone it stays; its copy matches on both strands and o = 0 is named
    x = rnd(k + 9, 4)
    s = x + rc(x)
    case("its own reverse complement, alone", [s], {})
    case("its own reverse complement, twice", [s, s], {1: (DUPLICATE, 0, 0, 0, 0)})
    # a palindromic anchor at even k ("ATATATAT" at k = 4): both orientations are candidates, one fits and matches
    pal = b"AT" * (k // 2) + (b"" if k % 2 == 0 else b"A")
    pu = pal + b"C" + rnd(k + 11, 5)
    pv = rnd(k + 3, 6) + b"G" + pu + b"G" + rnd(k + 8, 7)
    case("a palindromic anchor", [pu, pv], {0: (CONTAINED, 1, k + 4, 0, 0)})
    case("a palindromic anchor, flipped", [rc(pu), pv], {0: (CONTAINED, 1, k + 4, 1, 0)})
    # an anchor behind a leading N run; N against N is equal, N against A is not
    nu = b"N" * 70 + rnd(k + 13, 8)
    p, q = rnd(k + 2, 9), rnd(k + 5, 10)
    case("an anchor behind an N run, N equals N", [nu, p + nu + q], {0: (CONTAINED, 1, len(p), 0, 0)})
    na = p + b"A" + nu[1:] + q
    case("N against A is a mismatch", [nu, na], {})
    case("N against A is one mismatch", [nu, na], {0: (CONTAINED, 1, len(p), 0, 1)}, max_mismatches=1)
    case("N against A, flipped", [rc(nu), na], {0: (CONTAINED, 1, len(p), 1, 1)}, max_mismatches=1)
    # unanchored contigs are kept, equal ones too, and they have no window to contain anything with
    dense = (rnd(k - 1, 11) + b"N") * 4
    case("unanchored contigs stay", [b"ACGT", b"N" * (k + 10), b"", b"ACGT", b"", dense, dense, dense[:k + 5], rnd(2 * k, 12)], {})
    # a tandem repeat holds u at two positions: the smallest j
    t = rnd(k + 10, 13)
    case("twice in the container: the smallest j", [t, p + t + t + q], {0: (CONTAINED, 1, len(p), 0, 0)})
    case("twice in the container, flipped", [p + rc(t) + b"C" + rc(t) + q, t], {1: (CONTAINED, 0, len(p), 1, 0)})
    # the fit test one byte outside either end of the container: the window matches, j = -1 or j + L_u = L_v + 1; with one
    # mismatch allowed a comparison over the '_' would pass, the fit test does not
    f = rnd(2 * k + 6, 14)
    case("one byte in front of the container", [rnd(k, 15) + b"N", f + q, b"N" + f], {}, max_mismatches=1)
    case("one byte behind the container", [p + f, b"N" + rnd(k, 16), f + b"N"], {}, max_mismatches=1)
    case("one byte behind the container, flipped", [p + f, b"N" + rnd(k, 16), rc(f + b"N")], {}, max_mismatches=1)
    # KC_DEDUP_DUPLICATES_ONLY: a contained contig stays
    case("duplicates only", [b, b[:2 * k], b], {2: (DUPLICATE, 0, 0, 0, 0)}, duplicates_only=True)
    return out
