"""Host model of kc_fasta_to_block (include/kcount_mi355.h): the rules statement by statement, in plain
Python over bytes.  The device must equal it byte for byte; it is the tests' only reference."""
import numpy as np

OK, ERR_INVALID_ARG, ERR_CAPACITY, ERR_BAD_BASE = 0, -1, -6, -7
PARTIAL, STRICT = 1, 2
HDR_SCAN = 256
HAS_ID, HAS_DEPTH, LOWERED, RECODED = 1, 2, 4, 8
STATS = ("lines", "empty_lines", "records", "empty_records", "bases", "lowered", "recoded", "longest", "with_id", "with_depth")
REC_DTYPE = np.dtype([("hdr_pos", "<u8"), ("hdr_len", "<u4"), ("seq_lines", "<u4"), ("id", "<u8"), ("depth", "<u4"), ("flags", "<u4")])

PLAIN = b"ACGT"
LOWER = b"acgtn"
CODES = b"URYKMSWBDHV"
ACCEPTED = PLAIN + b"N" + LOWER + CODES
BLANKS = b"\r \t"


def split_lines(text):
    """[(begin, end)] of every line without its '\\n' and its trailing blanks; a last line may lack the '\\n'"""
    out, b = [], 0
    while b < len(text):
        e = text.find(b"\n", b)
        e = len(text) if e < 0 else e
        s = e
        while s > b and text[s - 1] in BLANKS:
            s -= 1
        out.append((b, s))
        b = e + 1
    return out


def consumed_of(text):
    """the position of the last '>' at a line's start, 0 when there is none"""
    at = 0
    for b, _ in split_lines(text):
        if b < len(text) and text[b:b + 1] == b">":
            at = b
    return at


def parse_header(h, default_depth=0):
    """(id, depth, flags) of a stripped header line h (with its '>')"""
    n = min(len(h), HDR_SCAN)
    is_open = len(h) > HDR_SCAN  # a token that reaches byte 256 does not end inside the bytes looked at
    ident, depth, flags = 0, default_depth, 0
    t1 = 1
    while t1 < n and h[t1] not in b" \t":
        t1 += 1
    if t1 == n and is_open:
        return ident, depth, flags
    nd = 0
    while t1 - nd > 1 and h[t1 - nd - 1:t1 - nd].isdigit():
        nd += 1
    if 1 <= nd <= 18:
        ident, flags = int(h[t1 - nd:t1]), flags | HAS_ID
    s2 = t1
    while s2 < n and h[s2] in b" \t":
        s2 += 1
    t2 = s2
    while t2 < n and h[t2] not in b" \t":
        t2 += 1
    if t2 > s2 and not (t2 == n and is_open):
        whole, dot, frac = h[s2:t2].partition(b".")
        digits = lambda s: all(48 <= c <= 57 for c in s)  # noqa: E731
        if 1 <= len(whole) <= 9 and digits(whole) and digits(frac):
            depth = min(65535, int(whole) + (1 if frac and frac[0] >= ord("5") else 0))
            flags |= HAS_DEPTH
    return ident, depth, flags


def parse(text, flags=0, default_depth=0):
    """-> dict(status, error, consumed, and on success seqs, offsets, depths, records, stats)"""
    text = bytes(text)
    strict = bool(flags & STRICT)
    used = consumed_of(text) if flags & PARTIAL else len(text)
    text = text[:used]
    accepted = (PLAIN + b"N") if strict else ACCEPTED
    errors = []  # (position, kind, message): the smallest wins, the structural one at one position
    recs, seqs, st = [], [], dict.fromkeys(STATS, 0)
    for no, (b, e) in enumerate(split_lines(text), 1):
        st["lines"] += 1
        if text[b:b + 1] == b">":
            ident, depth, fl = parse_header(text[b:e], default_depth)
            recs.append(dict(hdr_pos=b, hdr_len=e - b, seq_lines=0, id=ident, depth=depth, flags=fl))
            seqs.append(bytearray())
        elif e == b:
            st["empty_lines"] += 1
        else:
            if not recs:
                errors.append((b, 0, "fasta: line %d: sequence before the first header" % no))
            for p in range(b, e):
                c = text[p]
                if c not in accepted:
                    errors.append((p, 1, "fasta: line %d column %d: byte 0x%02x is not a base" % (no, p - b + 1, c)))
                    break
            if recs:
                r = recs[-1]
                r["seq_lines"] += 1
                for c in text[b:e]:
                    if c in LOWER:
                        r["flags"] |= LOWERED
                        st["lowered"] += 1
                    if c in CODES:
                        r["flags"] |= RECODED
                        st["recoded"] += 1
                    seqs[-1].append(c & 0xDF if (c & 0xDF) in PLAIN else ord("N"))
    if errors:
        _, kind, message = min(errors)
        return dict(status=ERR_INVALID_ARG if kind == 0 else ERR_BAD_BASE, error=message, consumed=used)
    block = b"".join(bytes(s) + b"_" for s in seqs)
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) + 1 for s in seqs], dtype=np.uint64)
    depths = np.concatenate([np.array([r["depth"]] * len(s) + [0], dtype=np.uint16) for r, s in zip(recs, seqs)] + [np.zeros(0, dtype=np.uint16)])
    records = np.zeros(len(recs), dtype=REC_DTYPE)
    for j, r in enumerate(recs):
        records[j] = tuple(r[k] for k in REC_DTYPE.names)
    st.update(records=len(recs), empty_records=sum(not s for s in seqs), bases=sum(len(s) for s in seqs), longest=max([len(s) for s in seqs] + [0]),
              with_id=sum(bool(r["flags"] & HAS_ID) for r in recs), with_depth=sum(bool(r["flags"] & HAS_DEPTH) for r in recs))
    status = ERR_CAPACITY if len(block) >= 1 << 31 else OK
    return dict(status=status, error=None, consumed=used, seqs=np.frombuffer(block, dtype=np.uint8), offsets=offsets, depths=depths, records=records,
                stats=st)
