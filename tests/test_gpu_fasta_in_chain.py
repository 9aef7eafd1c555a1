"""kc_fasta_to_block with what stands around it: the writer's text comes back as the block it was written from, a file streams
through load_contigs window by window, and the loaded block feeds the contig index and the contig k-mer pass as the
original does.  Expected values are the writer's model, the parser's model and the original block; never a second run of the
parser."""
import io

import numpy as np
import pytest

import asm_cases as AC
import asm_model as AM
import fasta_in_cases as FC
import fasta_in_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from test_gpu_asm import WIDTHS, on

pytestmark = pytest.mark.gpu


def host(a, dtype=None):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return a if dtype is None else a.view(dtype)


def equals_model(r, want, depths=True):
    assert (host(r["seqs"]) == want["seqs"]).all() and (host(r["offsets"], np.uint64) == want["offsets"]).all()
    assert host(r["records"], M.REC_DTYPE).tobytes() == want["records"].tobytes()
    if depths:
        assert (host(r["depths"], np.uint16) == want["depths"]).all()
    assert r["stats"] == want["stats"] and r["consumed"] == want["consumed"]


@pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))
def test_round_trip_of_the_writers_edge_block(dev):
    import torch
    seqs, offsets = AC.edge_block()
    n = len(offsets) - 1
    with pkg.KmerCounter(21) as kc:
        s, o = on(dev, seqs, offsets)
        for width in WIDTHS:
            text = kc.fasta_text(s, o, line_width=width)
            assert text == AM.fasta(seqs, offsets, None, "scaffold_", width)
            t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda() if dev else text
            r = kc.fasta_to_block(t)
            assert (host(r["seqs"]) == seqs).all() and (host(r["offsets"], np.uint64) == offsets).all()
            assert (host(r["records"], M.REC_DTYPE)["id"] == np.arange(n)).all() and r["depths"] is None
            out = io.BytesIO()
            kc.write_fasta(out, s, o, line_width=width, window_bytes=1000)
            r = kc.load_contigs(io.BytesIO(out.getvalue()), window_bytes=3000)
            assert (host(r["seqs"]) == seqs).all() and (host(r["offsets"], np.uint64) == offsets).all() and r["consumed"] == len(text)
        # a selection by length comes back under its ids
        order, _ = kc.select_contigs(s, o, min_len=16, by_length=True)
        r = kc.fasta_to_block(kc.fasta_text(s, o, order, line_width=60))
        assert (r["records"]["id"] == host(order, np.uint32)).all()
        want = AM.block([c.decode() for c in np.array(AM.contigs(seqs, offsets), dtype=object)[host(order, np.uint32)]])
        assert (r["seqs"] == want[0]).all() and (r["offsets"] == want[1]).all()


def test_streaming_equals_the_one_shot_parse():
    text = FC.edge_text("bases")
    want = M.parse(text, 0, 6)
    with pkg.KmerCounter(21) as kc:
        # smaller than the longest record: the window doubles; 97 and 1000 cut inside headers
        for window in (97, 1000, 70000, 1 << 20):
            r = kc.load_contigs(io.BytesIO(text), window_bytes=window, default_depth=6, with_depths=True)
            equals_model(r, want)
        # a refusal in a late window raises, whatever came before it
        with pytest.raises(pkg.KcError) as e:
            kc.load_contigs(io.BytesIO(text + b"\n>bad\nAC!\n"), window_bytes=70000)
        assert e.value.status == M.ERR_BAD_BASE and b"column 3: byte 0x21 is not a base" in pkg.lib().kc_last_error()
        # an empty file, and a file of one header
        r = kc.load_contigs(io.BytesIO(b""))
        assert r["seqs"].numel() == 0 and host(r["offsets"]).tolist() == [0] and r["records"].numel() == 0 and r["stats"]["records"] == 0
        r = kc.load_contigs(io.BytesIO(b">x_3 2"), with_depths=True)
        assert host(r["seqs"]).tobytes() == b"_" and host(r["offsets"]).tolist() == [0, 1] and host(r["depths"]).tolist() == [0]
        assert host(r["records"], M.REC_DTYPE)[0].tolist() == (0, 6, 0, 3, 2, 3)


def test_chain_loaded_contigs_align_as_the_original_block(tmp_path):
    import links_cases as LC
    from test_gpu_gap_align import block_arrays, read_arrays
    layout, _ = LC.LAYOUTS["gaps"]
    G = LC.genome(19)
    reads, _ = LC.pairs_of(G, 19)
    b, o = read_arrays(reads)
    seqs, offsets = block_arrays(LC.contigs_of(G, layout))
    with pkg.KmerCounter(LC.K) as kc:
        kc.index_contigs(seqs, offsets)
        want, want_first, want_stats = kc.align_reads(b, o)
        path = tmp_path / "contigs.fa"
        kc.write_fasta(str(path), seqs, offsets, line_width=70)
        r = kc.load_contigs(str(path), window_bytes=4096)
        assert (host(r["seqs"]) == host(seqs)).all() and (host(r["offsets"], np.uint64) == host(offsets, np.uint64)).all()
        kc.index_contigs(r["seqs"], r["offsets"])
        got, got_first, got_stats = kc.align_reads(b, o)
        assert len(want) > 100 and host(got).tobytes() == host(want).tobytes() and (host(got_first) == host(want_first)).all() and got_stats == want_stats


def test_depths_feed_the_contig_kmer_pass():
    import torch
    from close_cases import rand_seq
    rng = np.random.default_rng(29)
    ctgs = [rand_seq(rng, n) for n in (300, 77, 33, 1500, 40)]
    depth = [17, 3, 65535, 250, 0]
    text = b"".join(b">Contig%d %d.4\n" % (j, d) + AM.fasta(*AM.block([c]), None, "x", 60).split(b"\n", 1)[1] for j, (c, d) in enumerate(zip(ctgs, depth)))
    seqs, offsets = AM.block(ctgs)
    expanded = np.concatenate([np.array([d] * len(c) + [0], dtype=np.uint16) for c, d in zip(ctgs, depth)])
    reads = [c[i:i + 80] for c in ctgs for i in range(0, len(c) - 79, 9)] * 2
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in reads])
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    with pkg.KmerCounter(33) as kc, pkg.KmerCounter(33) as ref:
        for c in (kc, ref):
            c.submit_reads(bases, np.full(len(bases), ord("I"), dtype=np.uint8), offs)
        r = kc.fasta_to_block(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda(), with_depths=True)
        assert (host(r["seqs"]) == seqs).all() and (host(r["depths"], np.uint16) == expanded).all()
        kc.begin_ctg_kmers(len(seqs))
        kc.submit_ctg_block(r["seqs"], r["depths"])
        ref.begin_ctg_kmers(len(seqs))
        ref.submit_ctg_block(torch.from_numpy(seqs.copy()).cuda(), torch.from_numpy(expanded.view(np.int16).copy()).cuda())
        got, want = kc.sorted_results(), ref.sorted_results()
        assert kc.ctg_stats() == ref.ctg_stats() and len(want[1]) > 1000
        for g, w in zip(got, want):
            assert g.shape == w.shape and (g == w).all()


def test_wrapper_contract():
    import torch
    text = FC.small_text().replace(b"X", b"N")
    want = M.parse(text, 0, 5)
    with pkg.KmerCounter(21) as kc:
        h = kc.fasta_to_block(text, default_depth=5, with_depths=True)
        assert isinstance(h["seqs"], np.ndarray) and (h["seqs"].dtype, h["offsets"].dtype, h["depths"].dtype) == (np.uint8, np.uint64, np.uint16)
        assert h["records"].dtype == pkg.FASTA_REC_DTYPE and isinstance(h["consumed"], int) and list(h["stats"]) == list(M.STATS)
        equals_model(h, want)
        d = kc.fasta_to_block(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda(), default_depth=5, with_depths=True)
        assert all(d[k].is_cuda for k in ("seqs", "offsets", "depths", "records"))
        assert (d["seqs"].dtype, d["offsets"].dtype, d["depths"].dtype, d["records"].dtype) == (torch.uint8, torch.int64, torch.int16, torch.uint8)
        for k in ("seqs", "offsets", "depths", "records"):
            assert host(d[k]).tobytes() == h[k].tobytes(), k
        assert d["stats"] == h["stats"] and d["consumed"] == h["consumed"] == len(text)
        # numpy text, a str, the optional arrays left out, strict, partial
        r = kc.fasta_to_block(np.frombuffer(text, dtype=np.uint8), with_records=False)
        assert r["depths"] is None and r["records"] is None and (r["seqs"] == want["seqs"]).all()
        with pytest.raises(pkg.KcError) as e:
            kc.fasta_to_block(text, strict=True)
        assert e.value.status == M.ERR_BAD_BASE and pkg.lib().kc_last_error() == b"fasta: line 7 column 1: byte 0x61 is not a base"
        p = kc.fasta_to_block(text, partial=True)
        assert p["consumed"] == M.consumed_of(text) and len(p["offsets"]) == len(want["offsets"]) - 1
        # many more contigs than the first guess of the offsets' room
        many = b">\n" * 5000
        assert len(kc.fasta_to_block(many)["offsets"]) == 5001
        # no contigs, on either side
        for empty in (b"", torch.zeros(0, dtype=torch.uint8, device="cuda")):
            z = kc.fasta_to_block(empty, with_depths=True)
            assert len(z["seqs"]) == 0 and host(z["offsets"]).tolist() == [0] and len(z["depths"]) == 0 and len(z["records"]) == 0
            assert z["stats"] == dict.fromkeys(M.STATS, 0) and z["consumed"] == 0
        with pytest.raises(ValueError, match="default_depth"):
            kc.fasta_to_block(text, default_depth=70000)
