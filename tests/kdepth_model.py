"""Host model of kc_seq_kmer_depths and kc_count_spectrum (include/kcount_mi355.h); no tests here.

The rules are this project's own and this file pins them.  Everything is text: a window is k bytes that are all A C G T in
either case, inside one sequence; its key is the smaller of the upper-cased text and its reverse complement (A < C < G < T
is the order of the packed words); its count is that of the key among the results, 0 when it is not there.  The results
come in as (keys, counts) the way the oracle and KmerCounter.sorted_results() give them and are unpacked to text once.
"""
import numpy as np

REC_DTYPE = np.dtype([("sum", "<u8"), ("windows", "<u4"), ("present", "<u4"), ("solid", "<u4"), ("min_count", "<u2"), ("max_count", "<u2"),
                      ("mean", "<u2"), ("pad", "<u2", (3,))])
STATS = ("seqs", "bytes", "windows", "present", "solid", "sum", "longest")
SPECTRUM_STATS = ("kmers", "sum_counts", "max_count", "mode_count", "mode_kmers", "saturated")
BINS = 65536
FILL_MEAN = 1

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_UPPER = bytes.maketrans(b"acgt", b"ACGT")
_IS_BASE = np.zeros(256, dtype=bool)
_IS_BASE[list(b"ACGTacgt")] = True
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def revcomp(text):
    """of upper-case bytes; a byte that is no base stays as it is"""
    return text.translate(_COMP)[::-1]


def canonical(window):
    up = window.translate(_UPPER)
    return min(up, revcomp(up))


def key_texts(keys, k):
    """(n, words) packed keys -> n byte strings of k letters: base j in bits 63-2(j%32).. of word j/32"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(len(keys), -1)
    j = np.arange(k)
    codes = (keys[:, j // 32] >> (62 - 2 * (j % 32)).astype(np.uint64)) & np.uint64(3)
    text = _LETTERS[codes.astype(np.intp)]
    return [row.tobytes() for row in text]


def table(keys, counts, k):
    """the results as {canonical text: count}"""
    texts = key_texts(keys, k)
    tab = dict(zip(texts, (int(c) for c in counts)))
    assert len(tab) == len(texts), "a key twice among the results"
    return tab


def block(seqs):
    """strings or bytes -> (bytes u8, offsets u64) as the entry point takes them"""
    seqs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offsets


def mean_of(total, windows):
    return min(65535, (2 * total + windows) // (2 * windows)) if windows else 0


def kmer_depths(tab, k, seqs, offsets, min_count=0, fill_mean=False):
    """(track u16, records REC_DTYPE, stats dict) of the sequences seqs[offsets[i]:offsets[i+1]]"""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    n, nbytes = len(offsets) - 1, len(seqs)
    track = np.zeros(nbytes, dtype=np.uint16)
    recs = np.zeros(n, dtype=REC_DTYPE)
    stats = dict.fromkeys(STATS, 0)
    if n == 0 or nbytes == 0:
        return track, recs, stats
    assert int(offsets[0]) == 0 and int(offsets[n]) == nbytes and (np.diff(offsets.astype(np.int64)) >= 0).all()
    solid_at = max(min_count, 1)
    raw = seqs.tobytes()
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        stats["longest"] = max(stats["longest"], b - a)
        text = raw[a:b]
        base = _IS_BASE[seqs[a:b]]
        bad = np.concatenate(([0], np.cumsum(~base)))
        counts = []
        if b - a >= k:
            starts = np.flatnonzero(bad[k:] == bad[:b - a - k + 1])
            for p in starts:
                c = tab.get(canonical(text[p:p + k]), 0)
                counts.append(c)
                track[a + p] = c
        present = [c for c in counts if c]
        r = recs[i]
        r["sum"], r["windows"], r["present"] = sum(counts), len(counts), len(present)
        r["solid"] = sum(1 for c in counts if c >= solid_at)
        r["min_count"], r["max_count"] = (min(present), max(present)) if present else (0, 0)
        r["mean"] = mean_of(sum(counts), len(counts))
        if fill_mean:
            track[a:b] = np.where(base, r["mean"], 0)
    stats["seqs"], stats["bytes"] = n, nbytes
    for name in ("windows", "present", "solid", "sum"):
        stats[name] = int(recs[name].astype(np.uint64).sum())
    return track, recs, stats


def spectrum(counts):
    """(hist u64[BINS], stats dict) of the results' counts"""
    hist = np.bincount(np.asarray(counts, dtype=np.int64), minlength=BINS).astype(np.uint64)
    kmers = int(hist.sum())
    mode = int(np.argmax(hist)) if kmers else 0  # the first of equals: the smallest count
    stats = dict(kmers=kmers, sum_counts=int((hist * np.arange(BINS, dtype=np.uint64)).sum()),
                 max_count=int(np.flatnonzero(hist)[-1]) if kmers else 0, mode_count=mode, mode_kmers=int(hist[mode]) if kmers else 0,
                 saturated=int(hist[BINS - 1]))
    return hist, stats


def format_spectrum(hist):
    return "".join("%d %d\n" % (c, int(hist[c])) for c in range(len(hist)) if hist[c])


def unique_genome(rng, length, k):
    """random A C G T text in which no k-mer occurs twice, in either strand, and none is its own reverse complement"""
    while True:
        g = _LETTERS[rng.integers(0, 4, size=length)].tobytes()
        seen = set()
        for p in range(length - k + 1):
            w = g[p:p + k]
            rc = revcomp(w)
            if w == rc or w in seen or rc in seen:
                break
            seen.add(w)
        else:
            return g
