"""Plain-Python restatement of adapter trimming (kc_adapters_load / kc_trim_adapters, csrc/kc_trim.hpp): the reference's
Adapters::load_adapter_seqs, trim and trim_pair (src/adapters.cpp:48-146, 171-273) in the build it ships
(MERGE_READS_TRIM_WITH_SSW), and the part of its aligner that trim reads: ssw_align's score1, ref_begin1 and the three
end points (src/ssw/ssw_core.cpp:200-403, 874-955).  Scalar rules; only one column of the alignment matrix at a time is
a numpy vector.  Nothing here follows the aligner's striping: tests/golden/ssw_ref_alignments.json pins the values."""
import numpy as np

MAX_ADAPTER_K = 32     # src/adapters.hpp:56
STEP = 4               # src/adapters.cpp:183
MIN_TRIM_POS = 12      # :248
MAX_LEN = 32767        # kc_merge_pairs' read length limit
MAX_ENTRY_LEN = 1024   # kc_adapters_load's cap on an adapter's length
SCORES_ALTERNATE = (1, 1, 1, 1, 1)  # ALTERNATE_ALN_SCORES 11111: match, mismatch, gap open, gap extend, ambiguity
SCORES_BLASTN = (2, 3, 5, 2, 1)     # BLASTN_ALN_SCORES 23521


class BadBase(ValueError):
    pass


class UnsupportedK(ValueError):
    pass


class BadArg(ValueError):
    pass


# revcomp, src/utils.cpp:98-129
_COMP = {}
for _a, _b in zip("ACGTN", "TGCAN"):
    _COMP[ord(_a)] = _COMP[ord(_a.lower())] = ord(_b)
for _c in "URYKMSWBDHV":
    _COMP[ord(_c)] = ord("N")

# the 2-bit code of Kmer::get_kmers (src/kmer.cpp:191-192); bits 1 and 2 of the byte decide, so the case does not
KCODE = np.zeros(256, dtype=np.uint8)
for _c in range(256):
    _x = (_c & 4) >> 1
    KCODE[_c] = _x + ((_x ^ (_c & 2)) >> 1)

# kBaseTranslation (src/ssw/ssw.cpp:13-23): A C G T and U in either case, everything else 4; U shares A's code there
SSW_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    SSW_CODE[ord(_c)] = SSW_CODE[ord(_c.lower())] = _i
SSW_CODE[ord("U")] = SSW_CODE[ord("u")] = 0


def revcomp(seq):
    try:
        return bytes(_COMP[c] for c in reversed(seq))
    except KeyError:
        raise BadBase("revcomp: illegal byte")


def getlines(text):
    """the lines std::getline yields"""
    if not text:
        return []
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    return lines


class AdapterSet:
    def __init__(self, text, adapter_k, blastn_scores=False):
        if isinstance(text, str):
            text = text.encode()
        if adapter_k < 1 or adapter_k > MAX_ADAPTER_K:
            raise UnsupportedK("adapter_k %d" % adapter_k)
        self.k = adapter_k
        self.scores = SCORES_BLASTN if blastn_scores else SCORES_ALTERNATE
        self.entries = []
        self.n_short = 0
        for line in getlines(text):          # src/adapters.cpp:61-73
            if line[:1] == b">":
                continue
            if len(line) < adapter_k:
                self.n_short += 1
                continue
            if len(line) > MAX_ENTRY_LEN:
                raise BadArg("adapter longer than %d" % MAX_ENTRY_LEN)
            self.entries.append(bytes(line))
            self.entries.append(revcomp(line))
        self.index = {}                      # :118-131: k-mer -> [(entry, offset)] in insertion order
        for e, seq in enumerate(self.entries):
            codes = KCODE[np.frombuffer(seq, dtype=np.uint8)].tobytes()
            for j in range(len(seq) - adapter_k + 1):
                self.index.setdefault(codes[j:j + adapter_k], []).append((e, j))

    @property
    def n_adapters(self):
        return len(self.entries) // 2

    @property
    def n_kmers(self):
        return len(self.index)


def score_matrix(scores):
    """BuildSwScoreMatrix, src/ssw/ssw.cpp:25-49"""
    match, mismatch, _, _, amb = scores
    m = np.full((5, 5), -mismatch, dtype=np.int64)
    for i in range(4):
        m[i, i] = match
    m[4, :] = -amb
    m[:, 4] = -amb
    return m


def _sw_pass(q, ref, mat, go, ge, terminate):
    """One pass of the aligner over the columns `ref` (codes, in scan order) with the query codes `q` down the column.
    Returns (best score, index into ref of the ending column or -1, ending row)."""
    n = len(q)
    H = np.zeros(n, dtype=np.int64)
    E = np.zeros(n, dtype=np.int64)
    rows = np.arange(n, dtype=np.int64)
    best, end_col, hmax = 0, -1, None
    for idx, r in enumerate(ref):
        diag = np.empty(n, dtype=np.int64)
        diag[0] = 0
        diag[1:] = H[:-1]
        hpre = np.maximum(np.maximum(diag + mat[r][q], E), 0)
        # F(j) = max over j' < j of hpre(j') - go - (j - 1 - j') * ge: a gap down the column opens from a cell that
        # was not itself reached by such a gap (a longer gap is never worse than two)
        run = np.maximum.accumulate(hpre + rows * ge)
        F = np.full(n, -1, dtype=np.int64)
        F[1:] = run[:-1] - go - rows[:-1] * ge
        H = np.maximum(hpre, F)
        # ssw_core.cpp:295: E of the next column comes from H before F's correction
        E = np.maximum(E - ge, hpre - go)
        cm = int(H.max())
        if cm > best:                       # :336 strictly greater: the first column in scan order
            best, end_col, hmax = cm, idx, H
        if cm == terminate:                 # :352
            break
    end_row = 0 if hmax is None else int(np.argmax(hmax == best))  # :358-368 smallest row holding the maximum
    return best, end_col, end_row


def ssw_align(query, ref, scores):
    """Aligner::Align(query, ref, filter(report_cigar = false)): sw_score, ref_begin, ref_end, query_begin, query_end"""
    match, mismatch, go, ge, amb = scores
    mat = score_matrix(scores)
    q = SSW_CODE[np.frombuffer(bytes(query), dtype=np.uint8)].astype(np.int64)
    r = SSW_CODE[np.frombuffer(bytes(ref), dtype=np.uint8)].astype(np.int64)
    score, ref_end, q_end = _sw_pass(q, r, mat, go, ge, -1)
    # second pass (:936-951): the reversed query prefix against the reference from ref_end downwards, until a column's
    # maximum equals the score
    rq = q[:q_end + 1][::-1]
    rr = r[:ref_end + 1][::-1]
    _, rcol, rrow = _sw_pass(rq, rr, mat, go, ge, score)
    ref_begin = ref_end - rcol if rcol >= 0 else -1
    return {"sw_score": score, "ref_begin": ref_begin, "ref_end": ref_end, "query_begin": q_end - rrow, "query_end": q_end}


def trim(ads, seq):
    """Adapters::trim (src/adapters.cpp:171-258): (new length, trimmed, alignments)"""
    seq = bytes(seq)
    n = len(seq)
    k = ads.k
    best_identity, best_pos, found, nalign = 0.0, n, False, 0
    if n >= k:
        codes = KCODE[np.frombuffer(seq, dtype=np.uint8)].tobytes()
        matching = set()
        for i in range(0, n - k + 1, STEP):
            recs = ads.index.get(codes[i:i + k])
            if recs is None:
                continue
            for e, off in recs:
                if e in matching:
                    continue
                matching.add(e)
                ad = ads.entries[e]
                start = max(0, off - i - 2)
                ln = min(start + n + 2, len(ad))
                aln = ssw_align(ad[start:start + ln], seq, ads.scores)
                nalign += 1
                rb = aln["ref_begin"]
                mml = min(len(ad), n - rb if rb >= 0 else n + 1)
                identity = float(aln["sw_score"]) / float(ads.scores[0]) / float(mml)
                if identity >= best_identity:
                    best_identity, best_pos = identity, rb
                    if identity > 0.97:
                        found = True
                break
            if found:
                break
    if best_identity >= 0.5:
        if best_pos < MIN_TRIM_POS:
            best_pos = 0
        return best_pos, True, nalign
    return n, False, nalign


def trim_reads(ads, bases, quals, offsets, paired, per_read=None):
    """kc_trim_adapters: (bases, quals, offsets, stats) as numpy arrays and a dict.  per_read: a list that receives, or
    if filled already supplies, trim()'s answer for every read (the same for paired and unpaired mode)."""
    bases = np.asarray(bases, dtype=np.uint8)
    quals = np.asarray(quals, dtype=np.uint8)
    offsets = [int(o) for o in offsets]
    nreads = len(offsets) - 1
    if paired and nreads % 2:
        raise BadArg("odd number of reads")
    st = dict(reads=nreads, trimmed=0, bases_trimmed=0, reads_removed=0, alignments=0, out_bases=0)
    lens, flags = [], []
    for r in range(nreads):
        n = offsets[r + 1] - offsets[r]
        if n > MAX_LEN:
            raise BadArg("read longer than %d" % MAX_LEN)
        if not ads.entries:
            lens.append(n)
            flags.append(False)
            continue
        if per_read is not None and len(per_read) > r:
            ln, t, na = per_read[r]
        else:
            ln, t, na = trim(ads, bases[offsets[r]:offsets[r + 1]].tobytes())
            if per_read is not None:
                per_read.append((ln, t, na))
        st["alignments"] += na
        if t:
            st["trimmed"] += 1
            st["bases_trimmed"] += n - ln
            st["reads_removed"] += 1 if ln == 0 else 0
        lens.append(ln)
        flags.append(t)
    if paired:  # trim_pair, :260-273
        for p in range(0, nreads, 2):
            if (flags[p] or flags[p + 1]) and lens[p] > 1 and lens[p + 1] > 1:
                lens[p] = lens[p + 1] = min(lens[p], lens[p + 1])
    ob, oq, oo = [], [], [0]
    for r in range(nreads):
        ob.append(bases[offsets[r]:offsets[r] + lens[r]])
        oq.append(quals[offsets[r]:offsets[r] + lens[r]])
        oo.append(oo[-1] + lens[r])
    st["out_bases"] = oo[-1]
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.uint8)
    return cat(ob), cat(oq), np.array(oo, dtype=np.int64), st


# ---- the seeded inputs of tests/golden/ssw_ref_alignments.json -------------------------------------------------------
SSW_SEED = 20260117


def _rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def _mutate(rng, s, nsub, nindel):
    s = list(s)
    for _ in range(nsub):
        if s:
            p = int(rng.integers(0, len(s)))
            s[p] = "ACGT"[("ACGT".find(s[p].upper()) + 1 + int(rng.integers(0, 3))) % 4]
    for _ in range(nindel):
        if len(s) > 2:
            p = int(rng.integers(1, len(s) - 1))
            ln = int(rng.integers(1, 3))
            if rng.integers(0, 2):
                s[p:p] = list(_rand_seq(rng, ln))
            else:
                del s[p:p + ln]
    return "".join(s)


def _decorate(rng, s):
    """some Ns, IUPAC codes and lower case"""
    s = list(s)
    mode = int(rng.integers(0, 6))
    if mode == 0 and s:
        for _ in range(int(rng.integers(1, 4))):
            s[int(rng.integers(0, len(s)))] = "NnRYU"[int(rng.integers(0, 5))]
    elif mode == 1 and s:
        a = int(rng.integers(0, len(s)))
        b = int(rng.integers(a, len(s) + 1))
        s[a:b] = [c.lower() for c in s[a:b]]
    return "".join(s)


def ssw_cases(adapters, blastn):
    """The (query, ref) cases of one score set: adapters is the list of sequences of the committed adapter file."""
    rng = np.random.default_rng(SSW_SEED + (1 if blastn else 0))
    long_ads = [a for a in adapters if len(a) >= 50]
    out = []

    def pick(minlen=20):
        while True:
            a = adapters[int(rng.integers(0, len(adapters)))]
            if len(a) >= minlen:
                return a

    # adapter prefixes planted at every distance from the read's end, suffixes at the read's start
    for d in range(1, 151):
        for rep in range(8):
            a = pick()
            rl = 150
            read = _rand_seq(rng, rl - min(d, rl)) + a[:d]
            read = read[:rl]
            q = a[:min(len(a), d + 2 + int(rng.integers(0, 30)))]
            nsub, nind = int(rng.integers(0, 4)), int(rng.integers(0, 3)) if rep >= 5 else 0
            read = read[:rl - d] + _mutate(rng, read[rl - d:], nsub if d > 8 else 0, nind if d > 12 else 0)
            out.append((_decorate(rng, q), _decorate(rng, read)))
    for d in range(1, 120, 2):
        for rep in range(3):
            a = pick(40)
            suf = a[max(0, len(a) - d):]
            read = _mutate(rng, suf, int(rng.integers(0, 3)), 0) + _rand_seq(rng, int(rng.integers(20, 150)))
            out.append((_decorate(rng, a), _decorate(rng, read)))
    # homopolymer and dinucleotide repeats: ties, and gaps beside gaps
    for rep in range(900):
        unit = ["A", "C", "G", "T", "AC", "AG", "CT", "GT", "AT", "CG", "ACG", "AAC"][int(rng.integers(0, 12))]
        ql = int(rng.integers(1, 120))
        rl = int(rng.integers(5, 200))
        q = (unit * 200)[int(rng.integers(0, 3)):][:ql]
        r = (unit * 200)[int(rng.integers(0, 3)):][:rl]
        q = _mutate(rng, q, int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        r = _mutate(rng, r, int(rng.integers(0, 4)), int(rng.integers(0, 3)))
        if rep % 3 == 0:
            r = _rand_seq(rng, int(rng.integers(0, 40))) + r + _rand_seq(rng, int(rng.integers(0, 40)))
        out.append((_decorate(rng, q), _decorate(rng, r)))
    # low-complexity random pairs over small alphabets: many equal scores
    for rep in range(600):
        alpha = ["AC", "ACG", "ACGT", "AN", "ACGTN"][int(rng.integers(0, 5))]
        out.append((_rand_seq(rng, int(rng.integers(1, 60)), alpha), _rand_seq(rng, int(rng.integers(1, 160)), alpha)))
    # queries of 1-16, 17 and 119 bases
    for ql in list(range(1, 18)) * 12:
        a = pick()
        s = int(rng.integers(0, len(a) - min(ql, len(a)) + 1))
        q = a[s:s + ql]
        read = _rand_seq(rng, int(rng.integers(0, 100))) + _mutate(rng, q, int(rng.integers(0, 2)), 0) + _rand_seq(rng, int(rng.integers(0, 60)))
        out.append((_decorate(rng, q), _decorate(rng, read)))
    for rep in range(300):
        a = long_ads[int(rng.integers(0, len(long_ads)))]
        q = (a + _rand_seq(rng, 119))[:119]
        off = int(rng.integers(0, 150))
        read = (_rand_seq(rng, off) + _mutate(rng, q, int(rng.integers(0, 4)), int(rng.integers(0, 3))))[:150 + int(rng.integers(0, 120))]
        out.append((_decorate(rng, q), _decorate(rng, read)))
    # near-full matches of 110-119 bases and 200-base queries: with 2/3 scores max + bias crosses 255 both ways
    for rep in range(500):
        ql = int(rng.integers(110, 120)) if rep % 2 else 200
        q = _rand_seq(rng, ql)
        keep = int(rng.integers(ql - 30, ql + 1)) if rep % 4 < 2 else int(rng.integers(100, ql + 1))
        body = _mutate(rng, q[:keep], int(rng.integers(0, 6)), int(rng.integers(0, 3)))
        read = _rand_seq(rng, int(rng.integers(0, 60))) + body + _rand_seq(rng, int(rng.integers(0, 40)))
        out.append((_decorate(rng, q), _decorate(rng, read)))
    # unrelated sequences, and reads that score nothing
    for rep in range(200):
        out.append((_rand_seq(rng, int(rng.integers(1, 119))), _rand_seq(rng, int(rng.integers(1, 300)))))
    for rep in range(20):
        out.append(("N" * int(rng.integers(1, 30)), _rand_seq(rng, int(rng.integers(1, 50)), "ACGTN")))
        out.append((_rand_seq(rng, int(rng.integers(1, 30))), "N" * int(rng.integers(1, 50))))
    return out


def read_fasta_seqs(path):
    return [l.decode() for l in getlines(open(path, "rb").read()) if l[:1] != b">" and l]


def synthetic_adapters(seed=7, n=7500):
    """FASTA text of the shape of the reference's large adapter file: n sequences of 20-119 bases, a few shorter than
    any k in use, a few with IUPAC codes, some sharing long stretches with others (primer families)."""
    rng = np.random.default_rng(seed)
    out, seqs = [], []
    for i in range(n):
        kind = int(rng.integers(0, 40))
        if kind == 0:
            s = _rand_seq(rng, int(rng.integers(5, 17)))
        elif kind < 8 and seqs:  # a relative of an earlier sequence
            base = seqs[int(rng.integers(0, len(seqs)))]
            s = (_mutate(rng, base, int(rng.integers(0, 3)), 0) + _rand_seq(rng, int(rng.integers(0, 20))))[:119]
        else:
            s = _rand_seq(rng, int(rng.integers(20, 120)))
        if kind == 1 and len(s) > 4:
            s = list(s)
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, len(s)))] = "NRYKMSWBDHV"[int(rng.integers(0, 11))]
            s = "".join(s)
        seqs.append(s)
        out.append(">syn_%d\n%s\n" % (i, s))
    return "".join(out).encode()


_RC = str.maketrans("ACGT", "TGCA")


def random_pairs(seed, npairs, adapters, read_len=150, frag_lo=60, frag_hi=400, sub_rate=0.01, indel_rate=0.03, n_rate=0.03,
                 adapter_share=1.0):
    """Interleaved pairs of read_len bases from fragments of frag_lo .. frag_hi bases: a fragment shorter than the read
    is followed by an adapter (mate 1) or another one (mate 2), then random bases.  Returns (bases, quals, offsets)."""
    rng = np.random.default_rng(seed)
    bs, qs, offs = [], [], [0]
    for _ in range(npairs):
        flen = int(rng.integers(frag_lo, frag_hi + 1))
        frag = _rand_seq(rng, flen)
        for mate in range(2):
            ins = frag if mate == 0 else frag[::-1].translate(_RC)
            tail = ""
            if flen < read_len:
                if rng.random() < adapter_share:
                    tail = adapters[int(rng.integers(0, len(adapters)))]
                tail += _rand_seq(rng, read_len)
            r = (ins + tail)[:read_len]
            r = list(r)
            for p in np.nonzero(rng.random(len(r)) < sub_rate)[0]:
                r[p] = "ACGT"[int(rng.integers(0, 4))]
            if rng.random() < n_rate and r:
                r[int(rng.integers(0, len(r)))] = "N"
            r = "".join(r)
            if rng.random() < indel_rate and len(r) > 10:
                r = _mutate(rng, r, 0, 1)[:read_len]
            bs.append(r)
            qs.append(bytes(rng.integers(35, 74, len(r)).astype(np.uint8)))
            offs.append(offs[-1] + len(r))
    bases = np.frombuffer("".join(bs).encode(), dtype=np.uint8).copy()
    quals = np.frombuffer(b"".join(qs), dtype=np.uint8).copy()
    return bases, quals, np.array(offs, dtype=np.uint64)


# ---- per-read results and composed batches -----------------------------------------------------------------------------
def trim_per_read(ads, bases, offsets):
    """trim()'s answer for every read: [(new length, trimmed, alignments)], the per_read list of trim_reads"""
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = [int(o) for o in offsets]
    return [trim(ads, bases[offsets[r]:offsets[r + 1]].tobytes()) for r in range(len(offsets) - 1)]


class TrimItems:
    """The model's output read by read for a base set of reads.  Trimming is independent per pair when paired and per
    read when not, so the expected output of any arrangement of the base set's pairs (or reads) is a gather."""

    def __init__(self, ads, bases, quals, offsets, per_read=None):
        self.bases = np.asarray(bases, dtype=np.uint8)
        self.quals = np.asarray(quals, dtype=np.uint8)
        o = np.asarray(offsets).astype(np.int64)
        self.start, self.len = o[:-1], np.diff(o)
        self.per_read = per_read if per_read is not None else trim_per_read(ads, self.bases, o)
        self.cut = np.array([x[0] for x in self.per_read], dtype=np.int64)
        self.trimmed = np.array([x[1] for x in self.per_read], dtype=bool)
        self.naligns = np.array([x[2] for x in self.per_read], dtype=np.int64)
        n = len(self.len) // 2 * 2
        self.pair_len = self.cut.copy()  # final lengths under trim_pair's rule (an odd last read keeps its own)
        a, b = self.cut[0:n:2], self.cut[1:n:2]
        both = (self.trimmed[0:n:2] | self.trimmed[1:n:2]) & (a > 1) & (b > 1)
        self.pair_len[0:n:2] = np.where(both, np.minimum(a, b), a)
        self.pair_len[1:n:2] = np.where(both, np.minimum(a, b), b)

    def compose(self, order, paired):
        """order: pair indices when paired, read indices when not.  Returns (bases, quals, offsets u64, expected bases,
        expected quals, expected offsets int64, stats)."""
        from merge_model import gather_segments
        order = np.asarray(order, dtype=np.int64)
        reads = np.stack([2 * order, 2 * order + 1], axis=1).reshape(-1) if paired else order
        ln = self.len[reads]
        offs = np.zeros(len(reads) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(ln)
        bases = gather_segments(self.bases, self.start[reads], ln)
        quals = gather_segments(self.quals, self.start[reads], ln)
        fl = (self.pair_len if paired else self.cut)[reads]
        oo = np.zeros(len(reads) + 1, dtype=np.int64)
        oo[1:] = np.cumsum(fl)
        t = self.trimmed[reads]
        st = dict(reads=len(reads), trimmed=int(t.sum()), bases_trimmed=int((ln - self.cut[reads])[t].sum()),
                  reads_removed=int((t & (self.cut[reads] == 0)).sum()), alignments=int(self.naligns[reads].sum()), out_bases=int(oo[-1]))
        return bases, quals, offs, gather_segments(self.bases, self.start[reads], fl), gather_segments(self.quals, self.start[reads], fl), oo, st


# ---- seeded families aimed at the seed kernel's own structure ------------------------------------------------------------
def reads_to_arrays(reads, quals=None, seed=0):
    """[bytes / str] -> bases, quals (seeded 35..73 unless given), offsets u64"""
    reads = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    b = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    q = np.random.default_rng(seed).integers(35, 74, len(b)).astype(np.uint8) if quals is None else np.asarray(quals, dtype=np.uint8)
    return b, q, np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)


def _no_seed_filler(rng, ads, n):
    """n random bases none of whose k-mers is in the index (a fresh draw until that holds)"""
    while True:
        s = _rand_seq(rng, n)
        codes = KCODE[np.frombuffer(s.encode(), dtype=np.uint8)].tobytes()
        if all(codes[i:i + ads.k] not in ads.index for i in range(max(0, n - ads.k + 1))):
            return s


def seed_position_reads(ads, adapter, seed=61):
    """Reads holding exactly one k-mer of the index, the first k bases of `adapter`, at chosen positions: multiples of 4
    around the seed kernel's rounds of 224 bases, and their neighbours, which the stride of 4 never visits.  Returns
    [(read, position, position % 4 == 0)]."""
    rng = np.random.default_rng(seed)
    k = ads.k
    kmer = adapter[:k]
    out = []
    for ln in (k - 1, k, k + 1, 223 + k, 224 + k, 225 + k, 448 + k, 449 + k, 450 + k, 451 + k):
        if ln < k:
            out.append((_no_seed_filler(rng, ads, ln), -1, False))
            continue
        cand = [0, 4, 216, 220, 224, 228, 444, 448, ln - k]
        cand += [1, 2, 3, 5, 215, 217, 221, 222, 223, 225, 226, 227, 443, 445, 447, 449, ln - k - 1]
        for pos in sorted(set(c for c in cand if 0 <= c <= ln - k)):
            while True:
                s = _no_seed_filler(rng, ads, pos) + kmer + _no_seed_filler(rng, ads, ln - k - pos)
                codes = KCODE[np.frombuffer(s.encode(), dtype=np.uint8)].tobytes()
                hits = [i for i in range(ln - k + 1) if codes[i:i + k] in ads.index]
                if hits == [pos]:
                    break
            out.append((s, pos, pos % 4 == 0))
    return out
