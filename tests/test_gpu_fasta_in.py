"""kc_fasta_to_block (csrc/kc_fasta_in.hpp) against the host model tests/fasta_in_model.py, byte for byte: the block, the
offsets, the depths, the records, the statistics and `consumed`, from host arrays and from device tensors.  The model is never
replaced by a second device run.

Every call goes through fasta_in_cases.call: each output array is a slice of a larger poisoned array at a chosen byte offset,
of exactly the capacity, and the poison around it is checked there.

The edge text (fasta_in_cases.edge_text) holds line lengths 0, 1, 15, 16, 17, 31, 32 and 33; runs of empty records and of one-
to three-base contigs, so that several separators fall in one 16-byte chunk; CRLF and trailing blanks; every accepted byte of
the table; headers with and without id and depth (18- and 19-digit ids, 12.5, 12.49, 70000, 1e3, tokens across byte 256); one
200 000-base single line, longer than a tile of the line index; a header as the very last, unterminated line -- or, in its
second form, an unterminated last line of bases."""
import functools

import numpy as np
import pytest

import fasta_in_cases as FC
import fasta_in_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu
SIDES = pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))


@functools.lru_cache(maxsize=None)
def model(text, flags=0, default_depth=0):
    return M.parse(text, flags, default_depth)


def exact(kc, text, flags=0, default_depth=0, dev=False, **kw):
    """the call with arrays of exactly the model's sizes, against the model"""
    want = model(text, flags, default_depth)
    n, c = (len(want["seqs"]), len(want["offsets"]) - 1) if not want["status"] else (len(text), len(text))
    got = FC.call(kc, text, flags, default_depth, dev, seqs_capacity=n, ctgs_capacity=c, **kw)
    FC.same(got, want)
    return got


@SIDES
def test_edge_text_at_every_alignment(dev):
    with pkg.KmerCounter(21) as kc:
        for last in ("header", "bases"):
            text = FC.edge_text(last)
            for text_shift in range(16):
                exact(kc, text, 0, 9, dev, text_shift=text_shift, shift=(5 * text_shift + 1) % 16)
            for shift in (0, 1, 8, 15):
                exact(kc, text, 0, 65535, dev, text_shift=3, shift=shift)
        # without the optional arrays; the Python side
        want = model(FC.edge_text(), 0, 0)
        FC.same(FC.call(kc, FC.edge_text(), 0, 0, dev, shift=2, seqs_capacity=len(want["seqs"]), ctgs_capacity=len(want["offsets"]) - 1, depths=False,
                        records=False), want, depths=False, records=False)


@SIDES
def test_empty_inputs(dev):
    with pkg.KmerCounter(21) as kc:
        for text in (b"", b"\n", b"\n\r\n \t\n\n", b" ", b">", b">x", b">x\n", b">x\r\n\n", b">x 5\nA", b">\nA\n"):
            for flags in (0, M.PARTIAL):
                got = exact(kc, text, flags, 3, dev, shift=1)
                assert got["status"] == 0 and got["n_ctgs"] == (0 if flags else text.count(b">"))


@SIDES
def test_errors_leave_everything_untouched(dev):
    body = FC.edge_text("bases")
    cases = [(b">a\nXCGT\n>b\nAC\n", 0), (b">a\nACGT\n>b\nAC!", 0), (body + b"\n>z\nAC-GT\nA.C\n", 0), (b"\n \nACGT\n>a\nAC\n", 0),
             (b"ACGT\n>a\nA!C\n", 0), (b"AC!T\n>a\nAC\n", 0), (b"!CGT\n>a\n", 0), (b">a\nACgT\n", M.STRICT), (b">a\nACGT\nRACGT\n", M.STRICT),
             (b">a\nAC GT\n", 0), (b">a\n ACGT\n", 0), (b">a\nA>C\n", 0), (body + b"\nACG\x00", 0), (b">a\n" + b"ACGT" * 5000 + b"\x80" + b"ACGT" * 50, 0)]
    with pkg.KmerCounter(21) as kc:
        for text, flags in cases:
            want = model(text, flags)
            assert want["status"] in (M.ERR_BAD_BASE, M.ERR_INVALID_ARG)
            for text_shift in (0, 5):
                got = exact(kc, text, flags, 0, dev, text_shift=text_shift, shift=3)
                assert got["status"] == want["status"] and got["error"] == want["error"]
        # the exact strings, once by hand
        got = exact(kc, b">a\r\nACGT\r\nAC!T\r\nA!\r\n", 0, 0, dev)
        assert (got["status"], got["error"]) == (_lib.KC_ERR_BAD_BASE, "fasta: line 3 column 3: byte 0x21 is not a base")
        got = exact(kc, b"\nACGT\n>a\nA!\n", 0, 0, dev)
        assert (got["status"], got["error"]) == (_lib.KC_ERR_INVALID_ARG, "fasta: line 2: sequence before the first header")
        # strict refuses what the table recodes, and accepts ACGTN
        assert exact(kc, b">a\nACGTN\n", M.STRICT, 0, dev)["status"] == 0


@SIDES
def test_capacity(dev):
    text = FC.edge_text()
    want = model(text, 0, 4)
    n, c = len(want["seqs"]), len(want["offsets"]) - 1
    with pkg.KmerCounter(21) as kc:
        got = FC.call(kc, text, 0, 4, dev, query=True)
        assert got["status"] == 0 and "seqs" not in got
        FC.same(got, want)
        for dn, dc in ((-1, 0), (0, -1), (-n, 0), (0, -c)):
            got = FC.call(kc, text, 0, 4, dev, shift=7, seqs_capacity=n + dn, ctgs_capacity=c + dc)
            assert got["status"] == _lib.KC_ERR_CAPACITY and "%d contigs in %d bytes do not fit" % (c, n) in got["error"]
            assert (got["n_ctgs"], got["nbytes"], got["consumed"], got["stats"]) == (c, n, len(text), want["stats"])
        FC.same(FC.call(kc, text, 0, 4, dev, shift=7, seqs_capacity=n + 100, ctgs_capacity=c + 3), want)
        # a format error beats it
        bad = text + b"\nAC!\n"
        got = FC.call(kc, bad, 0, 4, dev, seqs_capacity=1, ctgs_capacity=0)
        FC.same(got, model(bad, 0, 4))
        assert got["status"] == _lib.KC_ERR_BAD_BASE


@SIDES
def test_partial_at_every_cut(dev):
    text = FC.small_text()
    with pkg.KmerCounter(21) as kc:
        seen = set()
        for cut in range(len(text) + 1):
            t = text[:cut]
            want = model(t, M.PARTIAL, 2)
            assert want["consumed"] == M.consumed_of(t)
            got = exact(kc, t, M.PARTIAL, 2, dev, text_shift=cut % 16, shift=cut % 7)
            # ... and equals the flag-free call on text[:consumed]
            flat = FC.call(kc, t[:want["consumed"]], 0, 2, dev, seqs_capacity=len(t), ctgs_capacity=len(t))
            assert flat["status"] == got["status"] and flat["error"] == got["error"]
            if not got["status"]:
                for k in ("seqs", "offsets", "depths", "records"):
                    assert flat[k].tobytes() == got[k].tobytes(), (cut, k)
                assert flat["stats"] == got["stats"]
            seen.add(got["status"])
        assert seen == {0, _lib.KC_ERR_BAD_BASE}  # the bad byte near the end is hidden until a header follows it
        assert exact(kc, text, 0, 2, dev)["status"] == _lib.KC_ERR_BAD_BASE
        # a partial text with a sequence in front of its first header, and one whose error lies behind the last header
        assert exact(kc, b"AC\n>a\nAC\n>b\n", M.PARTIAL, 0, dev)["status"] == _lib.KC_ERR_INVALID_ARG
        assert exact(kc, b">a\nAC\n>b\n!!\n", M.PARTIAL, 0, dev)["status"] == 0


@pytest.mark.parametrize("width", (60, 0))
def test_composed_scale(width):
    """about 300 000 contigs of 0 .. 2 000 bases: many workgroups in every kernel, more than one round of the scans"""
    import torch
    n = 300000
    text, seqs, offsets, lengths = FC.composed(13, n, 2000, width)
    with pkg.KmerCounter(21) as kc:
        r = kc.fasta_to_block(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda(), with_depths=True)
        assert r["consumed"] == len(text) and torch.equal(r["offsets"].cpu(), torch.from_numpy(offsets.view(np.int64)))
        got = r["seqs"].cpu().numpy()
        bad = np.flatnonzero(got != seqs)
        assert len(got) == len(seqs) and not len(bad), (len(got), len(seqs), bad[:3])
        ids = np.arange(n)
        depth = np.minimum(ids % 70000, 65535).astype(np.uint16)
        want_depths = np.repeat(depth, lengths + 1)
        want_depths[offsets[1:].astype(np.int64) - 1] = 0
        assert (r["depths"].cpu().numpy().view(np.uint16) == want_depths).all()
        recs = r["records"].cpu().numpy().view(M.REC_DTYPE)
        digits = np.char.str_len(ids.astype(str))
        assert (recs["id"] == ids).all() and (recs["depth"] == depth).all() and (recs["flags"] == 3).all()
        assert (recs["hdr_len"] == 4 + digits + np.char.str_len((ids % 70000).astype(str))).all()
        lines = np.where(lengths == 0, 0, 1 if not width else -(-lengths // max(width, 1)))
        assert (recs["seq_lines"] == lines).all()
        hdr_bytes = recs["hdr_len"].astype(np.int64) + 1
        seq_bytes = lengths + np.where(lengths == 0, 1, lines)  # an empty contig is written as one empty line
        starts = np.zeros(n, dtype=np.int64)
        starts[1:] = np.cumsum(hdr_bytes + seq_bytes)[:-1]
        assert (recs["hdr_pos"].astype(np.int64) == starts).all()
        st = r["stats"]
        assert st == dict(lines=int(n + np.where(lengths == 0, 1, lines).sum()), empty_lines=int((lengths == 0).sum()), records=n,
                          empty_records=int((lengths == 0).sum()), bases=int(lengths.sum()), lowered=0, recoded=0, longest=int(lengths.max()),
                          with_id=n, with_depth=n)
