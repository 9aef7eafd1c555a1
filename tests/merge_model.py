"""Plain-Python restatement of the pair merge (kc_merge_pairs, csrc/kc_merge.hpp): the pair loop of the reference's
merge_reads with no adapter file (src/merge_reads.cpp:469-648; Adapters::trim_pair returns at once without adapters,
src/adapters.cpp:260-261).  Written as the reference's sequential loop, side effects included; only the prefilter
(fast_count_mismatches, :195-236) is vectorised over the trial offsets with numpy."""
import json
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

_HERE = os.path.dirname(os.path.abspath(__file__))
Q2PERROR = [float(v) for v in json.load(open(os.path.join(_HERE, "golden", "q2perror.json")))["Q2Perror"]]

MIN_OVERLAP = 12            # merge_reads.cpp:344
EXTRA_TEST_OVERLAP = 2      # :345
MAX_MISMATCHES = 3          # :346
MAX_PERROR = 0.025          # :352
EXTRA_MISMATCHES_PER_1000 = 150  # :353
MAX_MATCH_QUAL = 41         # :354 (relative to qual_offset)
MAX_LEN = 32767             # int16_t lengths

# kc_fastq_to_packed's table (PackedRead, src/packed_reads.cpp:99-124)
CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _i
for _c in "NnURYKMSWBDHV":
    CODE[ord(_c)] = 4
# revcomp (src/utils.cpp:98-129): IUPAC -> N, lower case -> upper case
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip("ACGTN", "TGCAN"):
    COMP[ord(_a)] = COMP[ord(_a.lower())] = ord(_b)
for _c in "URYKMSWBDHV":
    COMP[ord(_c)] = ord("N")
N = ord("N")


class BadBase(ValueError):
    pass


class BadArg(ValueError):
    pass


def _check(seq, qual, qoff):
    if len(seq) > MAX_LEN:
        raise BadArg("mate longer than %d" % MAX_LEN)
    if len(seq) and (CODE[seq] == 255).any():
        raise BadBase("byte outside the table")
    q = qual.astype(np.int64) - qoff
    if len(q) and (q.min() < 0 or q.max() > 80):
        raise BadArg("quality outside [qual_offset, qual_offset + 80]")
    return [int(x) for x in q]


def prefilter_counts(s1, start, rc, length, ntr):
    """byte mismatches of every trial offset i < ntr: s1[start + i + j] vs rc[j], j < length - i"""
    seg = np.zeros(length + ntr, dtype=np.uint8)  # 0 never equals a byte of rc
    seg[:length] = s1[start:start + length]
    win = sliding_window_view(seg, length)[:ntr]
    return (win != rc[None, :length]).sum(axis=1) - np.arange(ntr)


def merge_pair(s1, q1a, s2, q2a, qoff=33, min_len=21):
    """One pair (numpy uint8 bases and ASCII qualities).  Returns (reads, st): reads a list of (bases bytes, relative
    qualities list) as they go into the read cache, st the pair's counters."""
    q1 = _check(s1, q1a, qoff)
    q2orig = _check(s2, q2a, qoff)
    st = dict(merged=0, ambiguous=0, dropped=0, overlap_len=0, merged_len=0)
    if len(s1) < min_len and len(s2) < min_len:  # :473
        st["dropped"] = 1
        return [], st
    rc = COMP[s2[::-1]]
    rq = q2orig[::-1]
    len1, len2 = len(s1), len(s2)
    length = min(len1, len2)
    start = len1 - length
    ntr = length - MIN_OVERLAP + EXTRA_TEST_OVERLAP
    best, found, abort, amb = -1, -1, False, 0
    mm = prefilter_counts(s1, start, rc, length, ntr) if ntr > 0 else []
    s1l, rcl = s1.tolist(), rc.tolist()
    for i in range(max(ntr, 0)):  # :494
        if abort:
            break
        overlap = length - i
        tmax = MAX_MISMATCHES + (EXTRA_MISMATCHES_PER_1000 * overlap // 1000)
        emax = tmax * 4 // 3 + 1
        if mm[i] > emax:  # fast_count_mismatches, :499-500
            continue
        matches = mism = both_ns = ncount = checked = 0
        perror = 0.0
        for j in range(overlap):  # :505-568
            checked += 1
            p = start + i + j
            ps, rs = s1l[p], rcl[j]
            if ps == rs:
                matches += 1
                if ps == N:
                    ncount += 2
                    both_ns += 1
                    if both_ns > 1:
                        abort = True
                        amb += 1
                        break
            else:
                mism += 1
                if ps == N:
                    mism += 1
                    ncount += 1
                    q1[p] = 0  # quals1[...] = qual_offset, :521
                    perror += Q2PERROR[rq[j]]
                elif rs == N:
                    ncount += 1
                    mism += 1
                    rq[j] = 0  # rev_quals2[j] = qual_offset, :529
                    perror += Q2PERROR[q1[p]]
                d = abs(q1[p] - rq[j])
                perror += 0.5 if d <= 2 else Q2PERROR[d]
            if ncount > 3:
                abort = True
                amb += 1
                break
            if mism > emax:
                break
        thres = max(overlap - tmax, MIN_OVERLAP)
        if matches >= thres and checked == overlap and mism <= tmax and perror / overlap <= MAX_PERROR:
            if best < 0 and found < 0:
                best = i
            else:
                amb += 1
                best = -1
                break
        elif checked == overlap and mism <= emax and perror / overlap <= MAX_PERROR * 4 / 3:
            found = i
            if best >= 0:
                amb += 1
                best = -1
                break
    st["ambiguous"] = amb
    if best >= 0 and not abort:  # :600-630
        overlap = length - best
        at = start + best
        seq, qual = list(s1l[:at]), list(q1[:at])
        for j in range(overlap):
            c1, c2, a, b = s1l[at + j], rcl[j], q1[at + j], rq[j]
            if c1 == c2:
                seq.append(c1)
                qual.append(min(a + b, MAX_MATCH_QUAL))
            else:
                seq.append(c2 if a < b else c1)
                qual.append(max(abs(a - b), 2))
        seq += rcl[overlap:]
        qual += rq[overlap:]
        st.update(merged=1, overlap_len=overlap, merged_len=len(seq))
        return [(bytes(seq), qual)], st
    return [(bytes(s1l), q1), (bytes(s2.tolist()), q2orig)], st


def pack(seq, qual):
    s = np.frombuffer(seq, dtype=np.uint8)
    return (CODE[s] | (np.minimum(np.asarray(qual, dtype=np.int64), 31).astype(np.uint8) << 3)).astype(np.uint8) if len(s) else \
        np.zeros(0, dtype=np.uint8)


def merge_pairs(bases, quals, offsets, qoff=33, min_len=21):
    """Interleaved pairs -> (packed u8, offsets u64, stats dict) of kc_merge_pairs."""
    bases = np.asarray(bases, dtype=np.uint8)
    quals = np.asarray(quals, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.uint64)
    npairs = (len(offsets) - 1) // 2
    st = dict(pairs=npairs, merged=0, ambiguous=0, dropped=0, overlap_len=0, merged_len=0, out_reads=0, out_bases=0)
    chunks, outo = [], [0]
    for p in range(npairs):
        o1, o2, e2 = (int(x) for x in offsets[2 * p:2 * p + 3])
        reads, ps = merge_pair(bases[o1:o2], quals[o1:o2], bases[o2:e2], quals[o2:e2], qoff, min_len)
        for k, v in ps.items():
            st[k] += v
        for seq, qual in reads:
            chunks.append(pack(seq, qual))
            outo.append(outo[-1] + len(seq))
    st["out_reads"] = len(outo) - 1
    st["out_bases"] = outo[-1]
    packed = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    return packed, np.array(outo, dtype=np.uint64), st


def packed_to_ascii(packed, offsets, qoff=33):
    """The read cache's bytes back to ASCII reads (ACGTN, qualities min(q, 31) + qoff): what the counting stage sees."""
    packed = np.asarray(packed, dtype=np.uint8)
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[packed & 7]
    quals = ((packed >> 3) + qoff).astype(np.uint8)
    return bases, quals, np.asarray(offsets, dtype=np.uint64)


def interleave(pairs):
    """[(seq1, qual1, seq2, qual2) as str / bytes] -> bases, quals, offsets of the interleaved layout"""
    b, q, o = [], [], [0]
    for pr in pairs:
        for s, qq in ((pr[0], pr[1]), (pr[2], pr[3])):
            s = s.encode() if isinstance(s, str) else bytes(s)
            qq = qq.encode() if isinstance(qq, str) else bytes(qq)
            assert len(s) == len(qq)
            b.append(s)
            q.append(qq)
            o.append(o[-1] + len(s))
    return (np.frombuffer(b"".join(b), dtype=np.uint8).copy(), np.frombuffer(b"".join(q), dtype=np.uint8).copy(),
            np.array(o, dtype=np.uint64))


def random_pairs(rng, npairs, min_len=1, max_len=300, qoff=33):
    """Seeded pairs of mixed lengths and overlaps: fragments cut from both ends, Ns, IUPAC and lower case, low-quality
    disagreements."""
    out = []
    for _ in range(npairs):
        l1 = int(rng.integers(min_len, max_len + 1))
        l2 = int(rng.integers(min_len, max_len + 1)) if rng.random() < 0.5 else l1
        frag = int(rng.integers(max(l1, l2), l1 + l2 + 20))
        g = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), frag)
        s1 = g[:l1].copy()
        s2 = COMP[g[frag - l2:][::-1]].copy()
        if rng.random() < 0.1:  # unrelated mate 2
            s2 = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), l2)
        q1 = rng.integers(2, 42, l1).astype(np.uint8)
        q2 = rng.integers(2, 42, l2).astype(np.uint8)
        for s, q in ((s1, q1), (s2, q2)):
            if len(s) == 0:
                continue
            nsub = rng.poisson(0.02 * len(s))
            for pos in rng.integers(0, len(s), nsub):
                s[pos] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8))
                q[pos] = rng.integers(0, 15)
            r = rng.random()
            if r < 0.15:
                for pos in rng.integers(0, len(s), rng.integers(1, 4)):
                    s[pos] = N
            elif r < 0.2:
                for pos in rng.integers(0, len(s), rng.integers(1, 3)):
                    s[pos] = rng.choice(np.frombuffer(b"acgtnRYKMSWBDHVU", dtype=np.uint8))
            if rng.random() < 0.02:
                q[:] = rng.integers(0, 81, len(q))
        out.append((s1.tobytes(), (q1 + qoff).tobytes(), s2.tobytes(), (q2 + qoff).tobytes()))
    return out
