"""Host model of kc_ctg_select and kc_fasta_text (include/kcount_mi355.h), written from the rules,
not from the kernels: pure Python and numpy, one statement a rule.  The device equals it byte for byte."""
import numpy as np

# kc_asm_stats in header order (ge_count and ge_bases are lists of len(CLASSES))
STATS = ("contigs", "bases", "selected", "sel_bases", "a", "c", "g", "t", "n", "n_runs", "longest", "shortest", "n50", "l50", "n90", "l90",
         "ge_count", "ge_bases", "key_bits")
CLASSES = (1000, 5000, 10000, 25000, 50000)
BY_LENGTH = 1
MAX_PREFIX = 32


def block(strings):
    """(seqs, offsets) of a seq block: every contig followed by '_'."""
    text = "".join(s + "_" for s in strings).encode()
    offsets = np.zeros(len(strings) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) + 1 for s in strings])
    return np.frombuffer(text, dtype=np.uint8).copy(), offsets


def contigs(seqs, offsets):
    """the contigs' byte strings"""
    raw = bytes(bytearray(seqs))
    return [raw[int(offsets[u]):int(offsets[u + 1]) - 1] for u in range(len(offsets) - 1)]


def nx(lengths_desc, x):
    """(Nx, Lx): Lx the smallest i with 100 S_i >= x T, Nx = l_Lx; (0, 0) without lengths"""
    total, s = sum(lengths_desc), 0
    for i, l in enumerate(lengths_desc, 1):
        s += l
        if 100 * s >= x * total:
            return l, i
    return 0, 0


def select(seqs, offsets, min_len=0, by_length=False):
    """-> (order as a list of block indices, stats dict with the keys of STATS)"""
    raw = bytes(bytearray(seqs))
    ctgs = contigs(seqs, offsets)
    chosen = [u for u, s in enumerate(ctgs) if len(s) >= min_len]
    ranked = sorted(chosen, key=lambda u: (-len(ctgs[u]), u))
    lens = [len(ctgs[u]) for u in ranked]
    st = dict.fromkeys(STATS, 0)
    st["contigs"], st["bases"] = len(ctgs), sum(len(s) for s in ctgs)
    st["selected"], st["sel_bases"] = len(chosen), sum(lens)
    arr = np.frombuffer(raw, dtype=np.uint8)
    flags = np.zeros(len(ctgs), dtype=bool)
    flags[chosen] = True
    counted = np.repeat(flags, np.diff(np.asarray(offsets).astype(np.int64)))  # a selected contig's positions; its '_' is no base
    for name in "acgtn":
        st[name] = int(((arr == ord(name.upper())) & counted).sum())
    is_n = arr == ord("N")
    first_of_run = is_n & np.concatenate(([True], ~is_n[:-1]))[:len(arr)]  # seqs[p] == 'N' and (p == 0 or seqs[p - 1] != 'N')
    st["n_runs"] = int((first_of_run & counted).sum())
    st["longest"], st["shortest"] = (lens[0], lens[-1]) if lens else (0, 0)
    (st["n50"], st["l50"]), (st["n90"], st["l90"]) = nx(lens, 50), nx(lens, 90)
    st["ge_count"] = [sum(1 for l in lens if l >= c) for c in CLASSES]
    st["ge_bases"] = [sum(l for l in lens if l >= c) for c in CLASSES]
    st["key_bits"] = (st["longest"] - st["shortest"]).bit_length()
    return (ranked if by_length else chosen), st


def record(u, seq, prefix, line_width):
    """one record: '>' prefix id '\\n', the bytes in lines of line_width (0: one line); an empty contig gives one empty line"""
    prefix = prefix.encode() if isinstance(prefix, str) else prefix
    lines = [seq[i:i + line_width] for i in range(0, len(seq), line_width)] if line_width and seq else [seq]
    return b">" + prefix + str(u).encode() + b"\n" + b"".join(l + b"\n" for l in lines)


def fasta(seqs, offsets, order=None, prefix="scaffold_", line_width=0):
    ctgs = contigs(seqs, offsets)
    order = range(len(ctgs)) if order is None else [int(u) for u in order]
    return b"".join(record(u, ctgs[u], prefix, line_width) for u in order)


def window(text, first_byte, capacity):
    """bytes [first_byte, min(total, first_byte + capacity)) of the text"""
    if first_byte > len(text):
        raise ValueError("first_byte %d is behind the text's %d bytes" % (first_byte, len(text)))
    return text[first_byte:first_byte + capacity]


def record_bytes(u, length, prefix_len, line_width):
    """1 + prefix_len + digits(u) + 1 + len + lines"""
    lines = max(1, -(-length // line_width)) if line_width else 1
    return 1 + prefix_len + len(str(u)) + 1 + length + lines
