"""tests/fasta_in_model.py against hand-written cases for every rule of kc_fasta_to_block's header comment, and against the
writer's model: asm_model.fasta then the parse gives the block back (no GPU needed)."""
import numpy as np
import pytest

import asm_cases as AC
import asm_model as AM
import fasta_in_cases as FC
import fasta_in_model as M

WIDTHS = (0, 1, 15, 16, 17, 60)
PREFIXES = ("", "scaffold_", "a-32-byte-prefix-for-the-records")


def block_of(r):
    return r["seqs"].tobytes()


def test_lines():
    # a line ends at '\n', the last line may lack it
    assert block_of(M.parse(b">a\nAC\n>b\nGT")) == b"AC_GT_"
    # trailing '\r', ' ' and '\t' are not part of a line
    r = M.parse(b">a \t\r\nAC\r\nG \t \r\n")
    assert block_of(r) == b"ACG_" and r["records"]["hdr_len"][0] == 2
    assert M.split_lines(b"ab \n\n c") == [(0, 2), (4, 4), (5, 7)]


def test_records():
    # a line whose first byte is '>' is a header and begins a record
    assert M.parse(b">a\n>b\n")["stats"]["records"] == 2
    # empty lines (after stripping) are ignored everywhere
    r = M.parse(b"\n \t\n>a\n\nAC\n\r\nGT\n  \n>b\n\n")
    assert block_of(r) == b"ACGT__" and r["stats"]["empty_lines"] == 6 and list(r["records"]["seq_lines"]) == [2, 0]
    # a record's sequence is the concatenation of its non-header lines up to the next header or the end of the text
    assert list(M.parse(b">a\nA\nC\nG\n>b\nT\nT")["offsets"]) == [0, 4, 7]
    # a header with no sequence gives an empty contig
    r = M.parse(b">a\n>b\nA\n>c")
    assert block_of(r) == b"_A__" and r["stats"]["empty_records"] == 2
    # a non-empty non-header line in front of the first header is a structural error, at its first byte
    r = M.parse(b"\n  \nAC\n>a\n")
    assert (r["status"], r["error"]) == (M.ERR_INVALID_ARG, "fasta: line 3: sequence before the first header")
    # a '>' that is not a line's first byte is no header
    assert M.parse(b">a\nA>C\n")["error"] == "fasta: line 2 column 2: byte 0x3e is not a base"


def test_alphabet():
    r = M.parse(b">a\nACGTacgt\nNnURYKMSWBDHV\n")
    # ACGT are copied, acgt become upper case, N n U R Y K M S W B D H V become N
    assert block_of(r) == b"ACGTACGT" + b"N" * 13 + b"_"
    assert (r["stats"]["lowered"], r["stats"]["recoded"], r["records"]["flags"][0]) == (5, 11, M.LOWERED | M.RECODED)
    # every other byte inside a sequence line is a bad base, interior white space included
    for c in range(256):
        ok = bytes([c]) in [bytes([x]) for x in M.ACCEPTED]
        r = M.parse(b">a\nA" + bytes([c]) + b"C\n")
        if c == 10:
            assert block_of(r) == b"AC_"
        else:
            assert (r["status"] == M.OK) == ok, c
            assert ok or r["error"] == "fasta: line 2 column 2: byte 0x%02x is not a base" % c
    # with KC_FASTA_STRICT everything but ACGTN is a bad base
    for c in M.ACCEPTED:
        r = M.parse(b">a\nAC" + bytes([c]), M.STRICT)
        assert (r["status"] == M.OK) == (c in b"ACGTN")
        assert r["status"] == M.OK or (r["status"], r["error"]) == (M.ERR_BAD_BASE, "fasta: line 2 column 3: byte 0x%02x is not a base" % c)


def test_errors():
    # the error at the smallest position wins, whichever kind it is
    assert M.parse(b"AC\n>a\nAXC\n")["error"] == "fasta: line 1: sequence before the first header"
    assert M.parse(b">a\nAXC\nAYZ\n")["error"] == "fasta: line 2 column 2: byte 0x58 is not a base"
    r = M.parse(b"AZ\n>a\n")
    assert (r["status"], r["error"]) == (M.ERR_INVALID_ARG, "fasta: line 1: sequence before the first header")
    # at one position, the structural one
    assert M.parse(b"Z\n")["status"] == M.ERR_INVALID_ARG
    # L and C are 1-based, C counts bytes from the line's start; blanks in front count
    r = M.parse(b">a\r\n\r\nACGT\r\n  ACG!\r\n")
    assert (r["status"], r["error"]) == (M.ERR_BAD_BASE, "fasta: line 4 column 1: byte 0x20 is not a base")
    assert "seqs" not in r


def test_output():
    r = M.parse(b">c1 3\nAC\n>c2\n>c3 2.5\nGGT\n", default_depth=9)
    assert block_of(r) == b"AC__GGT_" and list(r["offsets"]) == [0, 3, 4, 8]
    # depths: the record's depth on its bases and 0 on its separator
    assert list(r["depths"]) == [3, 3, 0, 0, 3, 3, 3, 0]
    assert r["stats"] == dict(lines=5, empty_lines=0, records=3, empty_records=1, bases=5, lowered=0, recoded=0, longest=3, with_id=3, with_depth=2)
    assert list(r["records"]["hdr_pos"]) == [0, 9, 13] and list(r["records"]["hdr_len"]) == [5, 3, 7] and list(r["records"]["depth"]) == [3, 9, 3]
    # the empty text, a text of only empty lines, only a header
    for t, n in ((b"", 0), (b"\n\r\n \n", 0), (b">x", 1), (b">x\n", 1)):
        r = M.parse(t)
        assert r["status"] == M.OK and list(r["offsets"]) == [0, 1][:n + 1] and block_of(r) == b"_" * n


def test_header_parse():
    for h, ident, depth, flags in FC.HEADERS:
        assert M.parse_header(h.rstrip(b" "), 77) == (ident, 77 if depth is None else depth, flags), h[:40]
    # the id is the maximal run of digits at the first token's end: 1 to 18 digits
    assert M.parse_header(b">Contig123 17.4") == (123, 17, 3)
    assert M.parse_header(b">12ab34") == (34, 0, 1) and M.parse_header(b">ab") == (0, 0, 0)
    assert M.parse_header(b">" + b"1" * 18)[0] == int("1" * 18) and M.parse_header(b">" + b"1" * 19) == (0, 0, 0)
    # the depth: 1 to 9 digits, optionally '.' and any number of digits; the first fractional digit rounds
    for tok, want in ((b"12.5", 13), (b"12.49", 12), (b"70000", 65535), (b"65534.5", 65535), (b"0", 0), (b"7.", 7), (b"999999999", 65535), (b"3.999", 4)):
        assert M.parse_header(b">x " + tok, 1) == (0, want, M.HAS_DEPTH), tok
    for tok in (b"1e3", b"1234567890", b".5", b"1.2.3", b"-1", b"1,5", b"x"):
        assert M.parse_header(b">x " + tok, 1) == (0, 1, 0), tok
    # only the first 256 bytes are looked at; a token that does not end inside them is absent
    assert M.parse_header(b">" + b"a" * 253 + b"1 5") == (1, 0, 1) and M.parse_header(b">" + b"a" * 254 + b"1 5") == (0, 0, 0)
    assert M.parse_header(b">" + b"a" * 254 + b"1") == (1, 0, 1)


def test_partial():
    t = b">a\nAC\n>b\nGT\n>c\nA!"
    # consumed is the position of the last '>' at a line's start; an error behind it is not reported
    r = M.parse(t, M.PARTIAL)
    assert (r["status"], r["consumed"], block_of(r)) == (M.OK, 12, b"AC_GT_") and M.parse(t)["status"] == M.ERR_BAD_BASE
    # 0 when there is none: KC_OK with 0 contigs, whatever the text holds
    r = M.parse(b"ACGT!\nAC", M.PARTIAL)
    assert (r["status"], r["consumed"], list(r["offsets"])) == (M.OK, 0, [0])
    # the call equals the flag-free call on text[0, consumed)
    for cut in range(len(t) + 1):
        p, q = M.parse(t[:cut], M.PARTIAL), M.parse(t[:M.consumed_of(t[:cut])])
        assert p["consumed"] == M.consumed_of(t[:cut]) and p["status"] == q["status"] and p["error"] == q["error"]
        assert p["status"] or (block_of(p) == block_of(q) and p["stats"] == q["stats"])
    # without the flag consumed = len
    assert M.parse(t[:12])["consumed"] == 12


@pytest.mark.parametrize("width", WIDTHS)
def test_the_writers_text_comes_back(width):
    seqs, offsets = AC.edge_block()
    n = len(offsets) - 1
    back = np.arange(n - 1, -1, -1, dtype=np.uint32)
    for prefix in PREFIXES:
        for order in (None, back):
            r = M.parse(AM.fasta(seqs, offsets, order, prefix, width))
            want_seqs, want_offsets = (seqs, offsets) if order is None else AM.block([c.decode() for c in AM.contigs(seqs, offsets)][::-1])
            assert r["status"] == M.OK and (r["seqs"] == want_seqs).all() and (r["offsets"] == want_offsets).all()
            assert list(r["records"]["id"]) == list(range(n) if order is None else back)
            assert (r["records"]["flags"] == M.HAS_ID).all() and r["stats"]["with_id"] == n


def test_the_edge_text_of_the_gpu_tests_holds_what_it_promises():
    for last in ("header", "bases"):
        t = FC.edge_text(last)
        r = M.parse(t)
        assert r["status"] == M.OK and (t[-1:] != b"\n")
        assert r["stats"]["longest"] == 200000 and r["stats"]["empty_records"] >= 5 and r["stats"]["lowered"] and r["stats"]["recoded"]
        assert set(M.ACCEPTED) <= set(t)
    by_header = {h.rstrip(b" "): (i, d, f) for h, i, d, f in FC.HEADERS}
    lines = M.split_lines(t)
    seen = 0
    for rec in M.parse(t, default_depth=77)["records"]:
        h = t[int(rec["hdr_pos"]):int(rec["hdr_pos"]) + int(rec["hdr_len"])]
        if h in by_header:
            i, d, f = by_header[h]
            assert (int(rec["id"]), int(rec["depth"]), int(rec["flags"]) & 3) == (i, 77 if d is None else d, f), h[:40]
            seen += 1
    assert seen == len(FC.HEADERS) and len(lines) > 150
    small = FC.small_text()
    assert 350 <= len(small) <= 450 and M.parse(small)["status"] == M.ERR_BAD_BASE
