"""tests/fastq_out_model.py against strings typed by hand for every rule of kc_fastq_text's header comment, against the
record-size formula, and through the library's host parsers: the model's text parses back to the arrays it was written
from (no GPU needed)."""
import numpy as np

import fastq_out_cases as FC
import fastq_out_model as M
import mhm2_kmer_analysis_v2_amd as pkg


def arrays(reads):
    """[(bases, quals)] as strings -> the front end's three arrays"""
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(b) for b, _ in reads])
    assert all(len(b) == len(q) for b, q in reads)
    return (np.frombuffer("".join(b for b, _ in reads).encode(), dtype=np.uint8).copy(),
            np.frombuffer("".join(q for _, q in reads).encode(), dtype=np.uint8).copy(), offsets)


FOUR = arrays([("ACGT", "IIII"), ("GGN", "#!~"), ("", ""), ("T", "5")])


def test_the_text_by_hand():
    b, q, o = FOUR
    assert M.fastq(b, q, o) == b"@r0\nACGT\n+\nIIII\n@r1\nGGN\n+\n#!~\n@r2\n\n+\n\n@r3\nT\n+\n5\n"
    # the reference's naming of pairs: both mates under the first one's index
    assert M.fastq(b, q, o, paired=True) == b"@r0/1\nACGT\n+\nIIII\n@r0/2\nGGN\n+\n#!~\n@r2/1\n\n+\n\n@r2/2\nT\n+\n5\n"
    assert M.fastq(b, q, o, order=[0, 2], paired=True) == b"@r0/1\nACGT\n+\nIIII\n@r2/1\n\n+\n\n"  # the mate-1 file
    assert M.fastq(b, q, o, order=[1, 3], paired=True, first_id=98) == b"@r98/2\nGGN\n+\n#!~\n@r100/2\nT\n+\n5\n"
    # an order: reversed, a repeat; ids; a prefix of none and of several bytes
    assert M.fastq(b, q, o, order=[3, 3, 1], prefix="") == b"@3\nT\n+\n5\n@3\nT\n+\n5\n@1\nGGN\n+\n#!~\n"
    ids = np.array([9, 10, 99, 10 ** 16 - 1], dtype=np.uint64)
    assert M.fastq(b, q, o, order=[3, 0], ids=ids, prefix="read_") == b"@read_9999999999999999\nT\n+\n5\n@read_9\nACGT\n+\nIIII\n"
    assert M.fastq(b, q, o, order=[1], ids=ids, paired=True) == b"@r10/2\nGGN\n+\n#!~\n"  # ids are taken as they are
    assert M.fastq(b, q, o, first_id=7, order=[2, 3]) == b"@r9\n\n+\n\n@r10\nT\n+\n5\n"
    assert M.fastq(b, q, o, order=[]) == b"" and M.fastq(*arrays([])) == b""


def test_packed_reads_by_hand():
    # code | quality << 3: A with 0, C with 1, G with 30, T with 31, N with 2, the codes 5 to 7 with 3
    packed = np.array([0 | 0 << 3, 1 | 1 << 3, 2 | 30 << 3, 3 | 31 << 3, 4 | 2 << 3, 5 | 3 << 3, 6 | 3 << 3, 7 | 3 << 3], dtype=np.uint8)
    o = np.array([0, 5, 8], dtype=np.uint64)
    assert M.fastq(packed, None, o) == b"@r0\nACGTN\n+\n!\"?@#\n@r1\nNNN\n+\n$$$\n"
    assert M.fastq(packed, None, o, qual_offset=64, order=[0]) == b"@r0\nACGTN\n+\n@A^_B\n"
    assert M.first_bad(packed, None, o) == (1, 1, "base", 0, 5 | 3 << 3) and M.first_bad(packed, None, o, order=[0, 0]) is None


def test_record_sizes_and_windows():
    b, q, o = FC.edge_reads()
    n = len(o) - 1
    ids = np.arange(n, dtype=np.uint64) * 10 ** 15 // 3
    for prefix in FC.PREFIXES:
        for paired in (False, True):
            for kw in (dict(first_id=0), dict(first_id=95), dict(ids=ids)):
                text = M.fastq(b, q, o, prefix=prefix, paired=paired, **kw)
                sizes = [M.record_bytes(int(o[i + 1] - o[i]), len(prefix), M.number(i, paired=paired, **kw), paired) for i in range(n)]
                assert len(text) == sum(sizes)
                at = 0
                for i, s in enumerate(sizes):
                    assert text[at:at + s] == M.record(b, q, o, i, prefix, paired=paired, **kw) and text[at:at + 1] == b"@"
                    at += s
    text = M.fastq(b, q, o, paired=True, first_id=8)
    order = list(range(n))
    for first, cap in ((0, 1), (0, len(text)), (5, 16), (len(text) - 3, 16), (len(text), 4), (4096, 4099), (70000, 1)):
        assert M.total_and_window(b, q, o, order, first, cap, paired=True, first_id=8) == (len(text), M.window(text, first, cap)), (first, cap)
    assert M.window(text, len(text), 5) == b"" and M.window(text, 3, 0) == b""


def test_check_names_the_first_byte_in_order():
    b, q, o = (x.copy() for x in FOUR)
    assert M.first_bad(b, q, o) is None
    q[5] = 0x20
    b[6] = 0x0A
    assert M.first_bad(b, q, o) == (1, 1, "base", 2, 0x0A)  # bases before qualities
    assert M.first_bad(b, q, o, order=[3, 0]) is None  # a read that the order leaves out
    q[0] = 0x7F
    assert M.first_bad(b, q, o, order=[3, 1, 0]) == (1, 1, "base", 2, 0x0A) and M.first_bad(b, q, o, order=[3, 0, 1]) == (1, 0, "quality", 0, 0x7F)


def test_the_text_parses_back_to_the_arrays():
    L = pkg.lib()
    assert hasattr(L, "kc_fastq_text")  # the writer this model pins
    b, q, o = FC.edge_reads()  # empty reads among them, an even count
    for prefix in ("r", ""):
        for paired in (False, True):
            text = M.fastq(b, q, o, prefix=prefix, paired=paired)
            gb, gq, go = pkg.fastq_pairs(text)
            assert (go == o).all() and (gb == b).all() and (gq == q).all()
    # a pair of files
    n = len(o) - 1
    t1, t2 = (M.fastq(b, q, o, order=range(m, n, 2), paired=True) for m in (0, 1))
    gb, gq, go = pkg.fastq_pairs(t1, t2)
    assert (go == o).all() and (gb == b).all() and (gq == q).all()
    # packed reads, codes <= 4: the parser packs the text into the bytes it was decoded from
    packed = FC.pack(b, q)
    gp, go = pkg.fastq_to_packed(M.fastq(packed, None, o), 33)
    assert (np.asarray(go) == o).all() and (np.asarray(gp) == packed).all()
    assert M.fastq(packed, None, o) == M.fastq(b, q, o)
