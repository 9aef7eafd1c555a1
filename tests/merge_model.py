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


def _prefilter_counts_whole(s1, start, rc, length, ntr):
    """prefilter_counts over one len x len window (kept to pin the row-block form against)"""
    seg = np.zeros(length + ntr, dtype=np.uint8)  # 0 never equals a byte of rc
    seg[:length] = s1[start:start + length]
    win = sliding_window_view(seg, length)[:ntr]
    return (win != rc[None, :length]).sum(axis=1) - np.arange(ntr)


def prefilter_counts(s1, start, rc, length, ntr, block_bytes=1 << 22):
    """byte mismatches of every trial offset i < ntr: s1[start + i + j] vs rc[j], j < length - i.  Worked in blocks of
    rows of about block_bytes comparisons, so that a mate of 32767 bases needs megabytes and not a gigabyte."""
    seg = np.zeros(length + ntr, dtype=np.uint8)  # 0 never equals a byte of rc
    seg[:length] = s1[start:start + length]
    win = sliding_window_view(seg, length)
    out = np.empty(ntr, dtype=np.int64)
    rows = max(1, block_bytes // max(length, 1))
    ref = rc[None, :length]
    for r0 in range(0, ntr, rows):
        r1 = min(ntr, r0 + rows)
        out[r0:r1] = (win[r0:r1] != ref).sum(axis=1)
    return out - np.arange(ntr)


def merge_pair(s1, q1a, s2, q2a, qoff=33, min_len=21):
    """One pair (numpy uint8 bases and ASCII qualities).  Returns (reads, st): reads a list of (bases bytes, relative
    qualities list) as they go into the read cache, st the pair's counters."""
    return merge_pair_ex(s1, q1a, s2, q2a, qoff, min_len)[:2]


# why the trial loop of a pair ended
STOP_RULES = ("dropped", "end", "abort_both_ns", "abort_ncount", "good_after_best", "good_after_weak", "weak_after_best")


def merge_pair_ex(s1, q1a, s2, q2a, qoff=33, min_len=21):
    """merge_pair, and as a third value the report of its trial loop: ntr (trials), stop (the offset of the last trial
    resolved, ntr - 1 when the loop ran out, -1 without a trial), rule (one of STOP_RULES), best (the merge offset or
    -1) and events, the deciding trials in offset order as (offset, "good" | "weak" | "abort")."""
    info = dict(ntr=0, stop=-1, rule="dropped", best=-1, events=[])
    q1 = _check(s1, q1a, qoff)
    q2orig = _check(s2, q2a, qoff)
    st = dict(merged=0, ambiguous=0, dropped=0, overlap_len=0, merged_len=0)
    if len(s1) < min_len and len(s2) < min_len:  # :473
        st["dropped"] = 1
        return [], st, info
    rc = COMP[s2[::-1]]
    rq = q2orig[::-1]
    len1, len2 = len(s1), len(s2)
    length = min(len1, len2)
    start = len1 - length
    ntr = length - MIN_OVERLAP + EXTRA_TEST_OVERLAP
    best, found, abort, amb = -1, -1, False, 0
    mm = prefilter_counts(s1, start, rc, length, ntr) if ntr > 0 else []
    s1l, rcl = s1.tolist(), rc.tolist()
    events = info["events"]
    info.update(ntr=max(ntr, 0), stop=max(ntr, 0) - 1, rule="end")
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
                        events.append((i, "abort"))
                        info.update(stop=i, rule="abort_both_ns")
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
                events.append((i, "abort"))
                info.update(stop=i, rule="abort_ncount")
                break
            if mism > emax:
                break
        thres = max(overlap - tmax, MIN_OVERLAP)
        if matches >= thres and checked == overlap and mism <= tmax and perror / overlap <= MAX_PERROR:
            events.append((i, "good"))
            if best < 0 and found < 0:
                best = i
            else:
                amb += 1
                info.update(stop=i, rule="good_after_best" if best >= 0 else "good_after_weak")
                best = -1
                break
        elif checked == overlap and mism <= emax and perror / overlap <= MAX_PERROR * 4 / 3:
            events.append((i, "weak"))
            found = i
            if best >= 0:
                amb += 1
                info.update(stop=i, rule="weak_after_best")
                best = -1
                break
    st["ambiguous"] = amb
    info["best"] = best if best >= 0 and not abort else -1
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
        return [(bytes(seq), qual)], st, info
    return [(bytes(s1l), q1), (bytes(s2.tolist()), q2orig)], st, info


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


# ---- per-pair results and composed batches -----------------------------------------------------------------------------
PAIR_STATS = ("merged", "ambiguous", "dropped", "overlap_len", "merged_len")


def gather_segments(data, starts, lens, chunk=1 << 15):
    """concatenation of data[starts[t] : starts[t] + lens[t]] over t, by numpy gathers of `chunk` segments at a time"""
    starts = np.asarray(starts, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    out = np.empty(int(lens.sum()), dtype=data.dtype)
    pos = 0
    for c0 in range(0, len(starts), chunk):
        ln = lens[c0:c0 + chunk]
        n = int(ln.sum())
        if n:
            idx = np.repeat(starts[c0:c0 + chunk] - (np.cumsum(ln) - ln), ln) + np.arange(n, dtype=np.int64)
            out[pos:pos + n] = data[idx]
            pos += n
    return out


class MergeItems:
    """The model's output pair by pair for a base set of pairs [(seq1, qual1, seq2, qual2)].  The merge is independent
    per pair, so the expected output of any arrangement of these pairs is a gather (compose)."""

    def __init__(self, pairs, qoff=33, min_len=21):
        self.qoff, self.min_len = qoff, min_len
        self.bases, self.quals, self.offsets = interleave(pairs)
        n = len(pairs)
        o = self.offsets.astype(np.int64)
        self.in_start = o[0:2 * n:2]
        self.len1 = o[1:2 * n:2] - o[0:2 * n:2]
        self.len2 = o[2:2 * n + 1:2] - o[1:2 * n:2]
        self.out_len = np.zeros((n, 2), dtype=np.int64)  # lengths of the pair's output reads (0: no such read)
        self.out_nreads = np.zeros(n, dtype=np.int64)
        self.stats = np.zeros((n, len(PAIR_STATS)), dtype=np.int64)
        self.info = []
        chunks = []
        for p in range(n):
            o1, o2, e2 = int(o[2 * p]), int(o[2 * p + 1]), int(o[2 * p + 2])
            reads, st, info = merge_pair_ex(self.bases[o1:o2], self.quals[o1:o2], self.bases[o2:e2], self.quals[o2:e2], qoff, min_len)
            self.info.append(info)
            self.stats[p] = [st[k] for k in PAIR_STATS]
            self.out_nreads[p] = len(reads)
            for r, (seq, qual) in enumerate(reads):
                chunks.append(pack(seq, qual))
                self.out_len[p, r] = len(seq)
        self.packed = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
        ob = self.out_len.sum(axis=1)
        self.out_start = np.cumsum(ob) - ob
        self.out_bytes = ob

    def __len__(self):
        return len(self.info)

    def is_long(self, cap=512):
        return np.maximum(self.len1, self.len2) > cap

    def compose(self, order):
        """(bases, quals, offsets u64, packed, out offsets u64, stats) of the arrangement order[0], order[1], ..."""
        order = np.asarray(order, dtype=np.int64)
        m = len(order)
        inlen = (self.len1 + self.len2)[order]
        bases = gather_segments(self.bases, self.in_start[order], inlen)
        quals = gather_segments(self.quals, self.in_start[order], inlen)
        rl = np.empty(2 * m, dtype=np.int64)
        rl[0::2] = self.len1[order]
        rl[1::2] = self.len2[order]
        offsets = np.zeros(2 * m + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(rl)
        packed = gather_segments(self.packed, self.out_start[order], self.out_bytes[order])
        ol = self.out_len[order].reshape(-1)
        keep = (np.arange(2)[None, :] < self.out_nreads[order][:, None]).reshape(-1)
        oo = np.zeros(int(keep.sum()) + 1, dtype=np.uint64)
        oo[1:] = np.cumsum(ol[keep])
        st = dict(zip(PAIR_STATS, (int(x) for x in self.stats[order].sum(axis=0))))
        st.update(pairs=m, out_reads=len(oo) - 1, out_bases=int(oo[-1]))
        return bases, quals, offsets, packed, oo, st


# ---- seeded families aimed at the kernels' own structure ----------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GRID_LENS = (1, 11, 12, 13, 63, 64, 65, 73, 74, 75, 127, 128, 129, 137, 138, 139, 255, 256, 257, 510, 511, 512, 513, 514, 516, 1000)
GRID_OFFSETS = (0, 1, 2, 3, 62, 63, 64, 65, 127, 128, 129)  # the ballot chunk edges, and every residue mod 4


def _other_base(rng, c):
    return ACGT[(int(np.nonzero(ACGT == c)[0][0]) + 1 + int(rng.integers(0, 3))) % 4]


def planted_pair(rng, len1, len2, i, qoff=33, nsub=0):
    """A pair whose true overlap is trial offset i: s1[start + i + j] == rc[j] for j < min(len1, len2) - i, but for nsub
    substitutions with far-apart qualities."""
    ln = min(len1, len2)
    start = len1 - ln
    s1 = rng.choice(ACGT, len1)
    rc = rng.choice(ACGT, len2)
    ov = ln - i
    s1[start + i:] = rc[:ov]
    q1 = rng.integers(20, 42, len1).astype(np.uint8)
    q2r = rng.integers(20, 42, len2).astype(np.uint8)
    for j in rng.integers(0, ov, nsub) if ov > 0 else ():
        s1[start + i + j] = _other_base(rng, rc[j])
        q1[start + i + j] = 3
    s2 = COMP[rc[::-1]]
    return (s1.tobytes(), (q1 + qoff).astype(np.uint8).tobytes(), s2.tobytes(), (q2r[::-1] + qoff).astype(np.uint8).tobytes())


def length_grid_pairs(seed=31, qoff=33):
    """Every (len1, len2) of GRID_LENS: a planted overlap at each offset of GRID_OFFSETS that leaves an overlap of at
    least 12, one unrelated pair (unmerged, or dropped when both mates are short), one overlap with substitutions."""
    rng = np.random.default_rng(seed)
    out = []
    for l1 in GRID_LENS:
        for l2 in GRID_LENS:
            ln = min(l1, l2)
            for i in GRID_OFFSETS:
                if ln - i >= MIN_OVERLAP:
                    while True:  # a chance second candidate among the shortest overlaps would make it ambiguous: draw again
                        pr = planted_pair(rng, l1, l2, i, qoff)
                        a = [np.frombuffer(x, dtype=np.uint8) for x in pr]
                        if max(l1, l2) < 21 or merge_pair_ex(a[0], a[1], a[2], a[3], qoff, 21)[2]["best"] == i:
                            break
                    out.append(pr)
            u = rng.choice(ACGT, l1 + l2)
            q = (rng.integers(2, 42, l1 + l2) + qoff).astype(np.uint8)
            out.append((u[:l1].tobytes(), q[:l1].tobytes(), u[l1:].tobytes(), q[l1:].tobytes()))
            if ln >= 40:
                out.append(planted_pair(rng, l1, l2, int(rng.integers(0, ln - 30)), qoff, nsub=3))
    return out


def _repeat(rng, p, n, phase=0):
    unit = rng.choice(ACGT, p)
    while p > 1 and (unit == unit[0]).all():
        unit = rng.choice(ACGT, p)
    return np.tile(unit, (n + phase) // p + 2)[phase:phase + n]


def _as_pair(s1, q1, rc, rq, qoff):
    return (s1.tobytes(), (q1 + qoff).astype(np.uint8).tobytes(), COMP[rc[::-1]].tobytes(), (rq[::-1] + qoff).astype(np.uint8).tobytes())


def cross_chunk_pairs(seed=41, n=1920, qoff=33):
    """Pairs of equal mates of 150-500 bases, s1 = A + X and rc = X + B with X the true overlap at offset len(A), built
    from unique and tandem-repeat stretches (periods 1-12) so that a second deciding trial falls into a later chunk of
    64 offsets than the first.  Six recipes in turn, about a third of the pairs still merge; classify_cross_chunk says
    from the model's trial report what a pair turned out to exercise."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        kind = t % 6
        ln = int(rng.integers(150, 501))
        p = int(rng.integers(1, 13))
        q1 = rng.integers(25, 42, ln).astype(np.uint8)
        rq = rng.integers(2, 12, ln).astype(np.uint8)  # far from q1: a mismatch costs next to nothing
        if kind == 0:  # unique overlap, true offset anywhere: merges
            i = int(rng.integers(0, ln - 40))
            x = rng.choice(ACGT, ln - i)
            s1 = np.concatenate([rng.choice(ACGT, i), x])
            rc = np.concatenate([x, rng.choice(ACGT, i)])
        elif kind == 1:  # unique stretch + repeat stretch, the unique one long enough that no shifted offset passes: merges
            i = int(rng.integers(64, ln - 100)) if ln > 170 else int(rng.integers(0, ln - 100))
            ov = ln - i
            u = int(rng.integers(60, ov - 20)) if ov > 85 else ov // 2
            x = np.concatenate([rng.choice(ACGT, u), _repeat(rng, p, ov - u)])
            s1 = np.concatenate([rng.choice(ACGT, i), x])
            rc = np.concatenate([x, rng.choice(ACGT, i)])
        elif kind == 2:  # repeat overlap whose first passing offset is the last of a chunk: the next one decides a chunk later
            p = int(rng.integers(4, 13))
            m = int(rng.integers(1, (ln - 40) // 64 + 1))
            i = 64 * m - 1
            ov = ln - i
            ext = _repeat(rng, p, ov + 24)  # the repeat, 12 bases further on both sides
            x = ext[12:12 + ov]
            a, b = rng.choice(ACGT, i), rng.choice(ACGT, i)
            for k in range(12):  # beside the overlap nothing continues the repeat, with equal qualities: earlier offsets fail
                a[i - 1 - k] = _other_base(rng, ext[11 - k])
                b[k] = _other_base(rng, ext[12 + ov + k])
            s1, rc = np.concatenate([a, x]), np.concatenate([x, b])
            q1[i - 12:i + 12] = 20
            rq[:12] = 20
            rq[ov - 12:ov + 12] = 20
            q1[ln - 12:] = 20
            for j in rng.integers(12, ov - 12, int(rng.integers(0, 3))):
                s1[i + j] = _other_base(rng, s1[i + j])
        elif kind == 3:  # the repeat runs d bases further left in mate 1; B starts with mismatches: weak trials, then a good one
            ov = int(rng.integers(40, 120))
            d = p * max(1, int(rng.integers(70, 150)) // p)
            if d + ov + 5 > ln:
                ln = d + ov + int(rng.integers(5, 40))
                q1 = rng.integers(25, 42, ln).astype(np.uint8)
                rq = rng.integers(2, 12, ln).astype(np.uint8)
            i = ln - ov
            ext = _repeat(rng, p, 2 * d + ov)
            tmax = MAX_MISMATCHES + EXTRA_MISMATCHES_PER_1000 * (ov + d) // 1000
            mm = tmax + 1 + int(rng.integers(0, 2))
            b = np.concatenate([ext[d + ov:2 * d + ov], rng.choice(ACGT, i - d)])
            for k in range(mm):
                b[k] = _other_base(rng, b[k])
            s1 = np.concatenate([rng.choice(ACGT, i - d), ext[:d + ov]])
            rc = np.concatenate([ext[d:d + ov], b])
        elif kind == 5:  # one repeat of a long period d >= 64: a single weak trial, the good one d offsets later and nothing between
            d = int(rng.integers(64, 141))
            ov = int(rng.integers(40, min(d, 120) + 1))
            iw = int(rng.integers(max(0, 150 - d - ov), 200))
            ln = iw + d + ov
            q1 = rng.integers(25, 42, ln).astype(np.uint8)
            rq = rng.integers(2, 12, ln).astype(np.uint8)
            u = rng.choice(ACGT, d)
            b = np.concatenate([u[ov:], u[:ov], rng.choice(ACGT, iw)])
            tmax = MAX_MISMATCHES + EXTRA_MISMATCHES_PER_1000 * (ov + d) // 1000
            for k in rng.choice(d, tmax + 1, replace=False):
                b[k] = _other_base(rng, b[k])
            s1 = np.concatenate([rng.choice(ACGT, iw), u, u[:ov]])
            rc = np.concatenate([u[:ov], b])
        else:  # four Ns inside a unique overlap at an offset of 64 or more: the pair aborts there
            i = int(rng.integers(64, ln - 40))
            ov = ln - i
            x = rng.choice(ACGT, ov)
            s1 = np.concatenate([rng.choice(ACGT, i), x])
            rc = np.concatenate([x, rng.choice(ACGT, i)])
            pos = rng.choice(ov, 4, replace=False)
            if t % 2:  # two matched Ns
                s1[i + pos[:2]] = N
                rc[pos[:2]] = N
            else:  # Ncount > 3
                s1[i + pos[:2]] = N
                rc[pos[2:]] = N
        out.append(_as_pair(s1, q1, rc, rq, qoff))
    return out


def classify_cross_chunk(info):
    """which of the cross-chunk kinds a pair's trial report shows (a set of names)"""
    kinds = set()
    ev = info["events"]
    if info["best"] >= 64:
        kinds.add("merged_late")
    goods = [i for i, k in ev if k == "good"]
    weaks = [i for i, k in ev if k == "weak"]
    if info["rule"] in ("good_after_best", "weak_after_best") and goods and goods[0] // 64 < info["stop"] // 64:
        kinds.add("best_then_later_chunk")
    if info["rule"] == "good_after_weak" and weaks and weaks[0] // 64 < info["stop"] // 64:
        kinds.add("weak_then_later_good")
    if info["rule"] == "good_after_weak" and weaks and max(weaks) // 64 < info["stop"] // 64:
        kinds.add("weak_only_in_earlier_chunks")  # nothing but the carried found_i makes this pair ambiguous
    if info["rule"] in ("abort_both_ns", "abort_ncount") and info["stop"] >= 64:
        kinds.add("abort_late")
    if any(k == "abort" and i >= 64 for i, k in ev) and any(k == "good" and i < 64 for i, k in ev):
        kinds.add("abort_late_after_early_good")
    return kinds


def long_path_pairs(seed=51, qoff=33):
    """The long-pair path's edges as a list of pairs (every one has a mate longer than 512 bases): mates at the documented
    limit of 32767, very unequal mates, lengths just over the static buffers, Ns, a best offset past 10 000."""
    rng = np.random.default_rng(seed)
    out = [planted_pair(rng, 32767, 32767, 0, qoff),       # full overlap at the limit
           planted_pair(rng, 32767, 13, 0, qoff),          # 32767 against 13
           planted_pair(rng, 13, 32767, 1, qoff),
           planted_pair(rng, 20000, 600, 3, qoff),         # both ways round
           planted_pair(rng, 600, 20000, 70, qoff),
           planted_pair(rng, 15000, 15000, 10007, qoff),   # best offset past 10 000
           planted_pair(rng, 12000, 11000, 10500, qoff, nsub=4)]
    for l in range(513, 521):                              # just over the static buffers
        out.append(planted_pair(rng, l, l, int(rng.integers(0, 400)), qoff))
        out.append(planted_pair(rng, l, 300, int(rng.integers(0, 200)), qoff))
        out.append(planted_pair(rng, 200, l, int(rng.integers(0, 150)), qoff, nsub=2))
    for ln, i in ((3000, 100), (5000, 4000), (700, 65)):   # Ns: the replay runs in dynamic LDS
        s1, qa, s2, qb = planted_pair(rng, ln, ln - 50, i, qoff, nsub=2)
        s1, s2 = bytearray(s1), bytearray(s2)
        s1[ln - 5] = N
        s2[len(s2) - 21] = N                               # position 20 of the reversed mate
        s1[3] = N                                          # outside the overlap: untouched by any trial
        out.append((bytes(s1), qa, bytes(s2), qb))
        s1[ln - 9] = N
        s2[len(s2) - 41] = N
        s2[len(s2) - 42] = N                                         # five Ns in the overlap: aborts
        out.append((bytes(s1), qa, bytes(s2), qb))
    u = rng.choice(ACGT, 1400)                             # unrelated long mates: unmerged
    q = (rng.integers(2, 42, 1400) + qoff).astype(np.uint8)
    out.append((u[:800].tobytes(), q[:800].tobytes(), u[800:].tobytes(), q[800:].tobytes()))
    return out
