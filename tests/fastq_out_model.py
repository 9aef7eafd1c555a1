"""Host model of kc_fastq_text (include/kcount_mi355.h), written from the rules, in plain Python: the
text record by record, a window of it, the record sizes by the formula, the first byte KC_FASTQ_OUT_CHECK refuses, and a
window of a text too large to build, from the records that overlap it.  Nothing in here calls the library."""
import bisect

import numpy as np

PACKED, PAIRED, CHECK = 1, 2, 4
MAX_PREFIX = 32
MAX_NUMBER = 9999999999999999
LETTERS = b"ACGTNNNN"


def read_bytes(bases, quals, offsets, i, qual_offset=33):
    """read i as (base line, quality line); quals None: bases holds packed bytes"""
    b = bytes(bytearray(bases[int(offsets[i]):int(offsets[i + 1])]))
    if quals is not None:
        return b, bytes(bytearray(quals[int(offsets[i]):int(offsets[i + 1])]))
    return bytes(LETTERS[x & 7] for x in b), bytes(((x >> 3) + qual_offset) & 0xFF for x in b)


def number(i, ids=None, first_id=0, paired=False):
    return int(ids[i]) if ids is not None else first_id + (i - (i & 1) if paired else i)


def name(i, prefix="r", ids=None, first_id=0, paired=False):
    prefix = prefix.encode() if isinstance(prefix, str) else prefix
    return b"@" + prefix + b"%d" % number(i, ids, first_id, paired) + ((b"/1", b"/2")[i & 1] if paired else b"")


def record(bases, quals, offsets, i, prefix="r", ids=None, first_id=0, paired=False, qual_offset=33):
    b, q = read_bytes(bases, quals, offsets, i, qual_offset)
    return name(i, prefix, ids, first_id, paired) + b"\n" + b + b"\n+\n" + q + b"\n"


def record_bytes(length, prefix_len, num, paired):
    return 6 + prefix_len + len(str(num)) + (2 if paired else 0) + 2 * length


def entries(offsets, order):
    return range(len(offsets) - 1) if order is None else [int(i) for i in order]


def fastq(bases, quals, offsets, order=None, prefix="r", ids=None, first_id=0, paired=False, qual_offset=33):
    """the whole text"""
    return b"".join(record(bases, quals, offsets, i, prefix, ids, first_id, paired, qual_offset) for i in entries(offsets, order))


def window(text, first_byte, capacity):
    return text[first_byte:first_byte + capacity]


def total_and_window(bases, quals, offsets, order, first_byte, capacity, prefix="r", ids=None, first_id=0, paired=False, qual_offset=33):
    """(the text's size, its bytes [first_byte, first_byte + capacity)) without the text: the records' sizes by the formula,
    their starts by addition, and only the records that overlap the window are formatted"""
    order = entries(offsets, order)
    plen = len(prefix.encode() if isinstance(prefix, str) else prefix)
    lens = np.diff(np.asarray(offsets).astype(np.int64))
    starts, at = [], 0
    for i in order:
        starts.append(at)
        at += record_bytes(int(lens[i]), plen, number(i, ids, first_id, paired), paired)
    if first_byte >= at or capacity <= 0:
        return at, b""
    j = bisect.bisect_right(starts, first_byte) - 1
    out, skip = b"", first_byte - starts[j]
    while j < len(order) and len(out) < skip + capacity:
        out += record(bases, quals, offsets, order[j], prefix, ids, first_id, paired, qual_offset)
        j += 1
    return at, out[skip:skip + capacity]


def first_bad(bases, quals, offsets, order=None):
    """what KC_FASTQ_OUT_CHECK refuses: (j, read, 'base' or 'quality', position, byte) of the first offending byte in (j, bases
    before qualities, position), or None"""
    for j, i in enumerate(entries(offsets, order)):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        for which, arr in (("base", bases), ("quality", quals)):
            if arr is None:
                continue
            for pos, x in enumerate(bytearray(arr[lo:hi])):
                if ((x & 7) > 4) if quals is None else not 0x21 <= x <= 0x7E:
                    return j, i, which, pos, x
    return None
