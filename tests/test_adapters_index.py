"""kc_adapters_index (host only, no GPU) against tests/trim_model.py's loader: Adapters::load_adapter_seqs
(src/adapters.cpp:48-146)."""
import os

import pytest

import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

import trim_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FA = open(os.path.join(GOLD, "adapters_no_transposase.fa"), "rb").read()


def same(text, k):
    got = pkg.adapters_index(text, k)
    m = M.AdapterSet(text, k)
    assert got == dict(n_adapters=m.n_adapters, n_short=m.n_short, n_entries=len(m.entries), n_kmers=m.n_kmers), (k, got)
    return got


def test_symbols_resolve():
    L = pkg.lib()
    for name in ("kc_adapters_index", "kc_adapters_load", "kc_adapters_clear", "kc_trim_adapters"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert L.kc_abi_version() == 1


@pytest.mark.parametrize("k", [17, 21, 31, 32])
def test_committed_adapter_file(k):
    got = same(FA, k)
    assert got["n_adapters"] + got["n_short"] == 154 and got["n_kmers"] > 1000


def test_synthetic_big_set():
    text = M.synthetic_adapters()
    got = same(text, 21)
    assert got["n_short"] > 50 and got["n_adapters"] > 7000 and got["n_kmers"] > 400000
    same(text, 32)


@pytest.mark.parametrize("text", [
    b"",
    b">only a name",
    b">only a name\n",
    b">a\nACGTACGTACGTACGTACGTACGT",            # no trailing newline
    b">a\nACGTACGTACGTACGTACGTACGT\n\n",        # an empty line counts as a short sequence
    b"\n\n\n",
    b">a\nACGT\n>b\nACGTACGTACGTACGTACGTA\n",    # shorter than k, exactly k
    b"ACGTNNNNRYKMSWBDHVUacgtnACGT\nacgtacgtacgtacgtacgtacgtacgt\n",  # IUPAC and lower case, no name lines
    b">a\nAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA\n>b\nTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT\n",  # shared k-mers, both strands
    b">a\nGGGGGGGGGGGGGGGGGGGGGGGGG\n>b\nNNNNNNNNNNNNNNNNNNNNNNNNNNN\n",  # N counts as G
])
def test_corner_texts(text):
    same(text, 21)


def status_of(text, k):
    with pytest.raises(pkg.KcError) as e:
        pkg.adapters_index(text, k)
    return e.value.status


def test_errors():
    assert status_of(b">a\nACGTACGTACGTACGTACGTACGT\r\n", 21) == _lib.KC_ERR_BAD_BASE  # the CR is part of the sequence
    with pytest.raises(M.BadBase):
        M.AdapterSet(b">a\nACGTACGTACGTACGTACGTACGT\r\n", 21)
    assert status_of(b">a\nACGTACGTACGTACGTACGTACGT\r", 21) == _lib.KC_ERR_BAD_BASE
    same(b">a\r\nACGT\r\n", 21)  # a CR on a name line or in a short sequence is never looked at
    assert status_of(b">a\nACGTACGTACGTACGTACGT-CGT\n", 21) == _lib.KC_ERR_BAD_BASE
    assert status_of(b">a\nACGTACGTACGTACGTACGTuCGT\n", 21) == _lib.KC_ERR_BAD_BASE  # revcomp takes U, not u
    assert status_of(FA, 33) == _lib.KC_ERR_UNSUPPORTED_K
    assert status_of(FA, 0) == _lib.KC_ERR_INVALID_ARG
    assert status_of(b">a\n" + b"ACGT" * 257 + b"\n", 21) == _lib.KC_ERR_INVALID_ARG  # longer than the cap of 1024
    same(b">a\n" + b"ACGT" * 256 + b"\n", 21)
