"""Host model of kc_shuffle_reads (csrc/kc_shuffle.hpp): the definitions of include/kcount_mi355.h and DESIGN.md section 22
in plain Python, a loop over the pairs with no cleverness.  The reference holds no code for the step, so this file IS
the definition the device is compared with, byte for byte; tests/test_shuffle_model.py checks it against cases whose
answer follows from the case alone.

Contigs are given by their lengths only (the call never reads a contig's base); reads by their bytes."""
import numpy as np

from depth_model import MAX_READ_LEN, NO_ALN, PAIR_DTYPE, BadArg, BadRead, BadRecord, check_records, pair_inserts, rec, records  # noqa: F401
from gap_model import GAP_ALN_DTYPE, KIND_NONE  # noqa: F401
from lassm_model import BadPair, check_pairs  # noqa: F401

MAX_PARTS = 65536
NO_HOME = 0xFFFFFFFF
SHUFFLE_STATS = ("pairs", "homed", "homeless", "one_mate", "two_same", "two_diff", "homes", "max_home_pairs", "bytes", "key_bits")


def choose(c0, c1):
    """the chosen record of a pair's candidates (None: none): the first by (greater score, smaller ctg, smaller cstart,
    mate 0 before mate 1)"""
    cands = [(-int(c["score"]), int(c["ctg"]), int(c["cstart"]), mate) for mate, c in ((0, c0), (1, c1)) if c is not None]
    if not cands:
        return None
    return (c0, c1)[min(cands)[3]]


def deal(nh, nu, parts):
    """rule 3: (slots, part_starts); slots[q] = (homed?, rank within its segment) of new pair q"""
    slots, starts = [], []
    for j in range(parts):
        starts.append(len(slots))
        slots += [(True, r) for r in range(j * nh // parts, (j + 1) * nh // parts)]
        slots += [(False, r) for r in range(j * nu // parts, (j + 1) * nu // parts)]
    starts.append(len(slots))
    return slots, starts


def key_bits(ctg_lens, npairs):
    """the bits the sort runs over: the anchor field has the bit length of the longest contig, the home field that of n_ctgs
    (a homeless pair holds n_ctgs there); no pairs, no sort"""
    if not npairs:
        return 0
    return max(ctg_lens, default=0).bit_length() + len(ctg_lens).bit_length()


def shuffle_reads(ctg_lens, bases, quals, offsets, alns, pairs, parts=1):
    """kc_shuffle_reads: a dict of the outputs as bytes (quals None without qualities; gap_alns and pairs always, a caller
    compares what it asked for) and stats as a dict.  bases / quals: bytes; offsets: nreads + 1 integers."""
    nreads = len(offsets) - 1
    if nreads & 1:
        raise BadArg("%d reads are no pairs" % nreads)
    if not 1 <= parts <= MAX_PARTS:
        raise BadArg("parts %d outside 1 .. %d" % (parts, MAX_PARTS))
    offsets = [int(x) for x in offsets]
    for r in range(nreads):
        if offsets[r + 1] < offsets[r] or offsets[r + 1] - offsets[r] > MAX_READ_LEN:
            raise BadRead(r)
    read_lens = [offsets[r + 1] - offsets[r] for r in range(nreads)]
    check_records(alns, ctg_lens, read_lens, nreads)
    check_pairs(pairs, alns, nreads)
    npairs = nreads // 2
    st = dict.fromkeys(SHUFFLE_STATS, 0)
    st["pairs"], st["bytes"], st["key_bits"] = npairs, offsets[nreads], key_bits(ctg_lens, npairs)
    # rule 1: the homes
    homed, homeless = [], []
    for p in range(npairs):
        c = [None if int(pairs[p][n]) == NO_ALN else alns[int(pairs[p][n])] for n in ("aln0", "aln1")]
        b = choose(*c)
        if b is None:
            homeless.append(p)
            continue
        homed.append((int(b["ctg"]), int(b["cstart"]), p))
        if c[0] is None or c[1] is None:
            st["one_mate"] += 1
        elif int(c[0]["ctg"]) == int(c[1]["ctg"]):
            st["two_same"] += 1
        else:
            st["two_diff"] += 1
    # rule 2: the order within a segment
    homed.sort()
    st["homed"], st["homeless"] = len(homed), len(homeless)
    per_home = {}
    for h, _, _ in homed:
        per_home[h] = per_home.get(h, 0) + 1
    st["homes"], st["max_home_pairs"] = len(per_home), max(per_home.values(), default=0)
    # rule 3: the parts
    slots, starts = deal(len(homed), len(homeless), parts)
    order = [homed[r][2] if is_homed else homeless[r] for is_homed, r in slots]
    home = [homed[r][0] if is_homed else NO_HOME for is_homed, r in slots]
    assert len(order) == npairs
    # rule 4: the outputs
    new_of = {p: q for q, p in enumerate(order)}
    new_offsets, out_b, out_q = [0], [], []
    for p in order:
        for r in (2 * p, 2 * p + 1):
            out_b.append(bytes(bases[offsets[r]:offsets[r + 1]]))
            if quals is not None:
                out_q.append(bytes(quals[offsets[r]:offsets[r + 1]]))
            new_offsets.append(new_offsets[-1] + read_lens[r])
    alns_out = np.array(alns, dtype=GAP_ALN_DTYPE)
    for i in range(len(alns_out)):
        r = int(alns_out[i]["read"])
        alns_out[i]["read"] = 2 * new_of[r >> 1] + (r & 1)
    pairs_out = np.array([pairs[p] for p in order], dtype=PAIR_DTYPE) if npairs else np.zeros(0, dtype=PAIR_DTYPE)
    return {"bases": b"".join(out_b), "quals": None if quals is None else b"".join(out_q),
            "offsets": np.array(new_offsets, dtype=np.uint64).tobytes(), "order": np.array(order, dtype=np.uint32).tobytes(),
            "home": np.array(home, dtype=np.uint32).tobytes(), "part_starts": np.array(starts, dtype=np.uint64).tobytes(),
            "gap_alns": alns_out.tobytes(), "pairs": pairs_out.tobytes(), "stats": st}
