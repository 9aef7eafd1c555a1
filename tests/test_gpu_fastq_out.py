"""kc_fastq_text (csrc/kc_fastq_out.hpp) against the host model tests/fastq_out_model.py, byte for byte: the text whole and
window by window, from host arrays and from device tensors, ASCII and packed, and back through the device's own parsers.
The model is never replaced by a second device run.

Every text call goes through fastq_out_cases.text_call: `text` is a slice of a larger poisoned array at a chosen byte offset,
of exactly the capacity, the source arrays begin at a byte shift of their allocation, and the bytes in front of and behind
the window must stay poisoned."""
import functools
import io

import numpy as np
import pytest

import fastq_out_cases as FC
import fastq_out_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from fastq_out_cases import on, text_call
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

E, CAP, BAD = _lib.KC_ERR_INVALID_ARG, _lib.KC_ERR_CAPACITY, _lib.KC_ERR_BAD_BASE
DEVS = pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))
PACKS = pytest.mark.parametrize("packed", (False, True), ids=("ascii", "packed"))


def source(reads, packed):
    """(bases, quals) as the call takes them"""
    b, q, _ = reads
    return (FC.pack(b, q), None) if packed else (b, q)


@functools.lru_cache(maxsize=None)
def edge_text(packed, paired, prefix):
    b, q = source(FC.edge_reads(), packed)
    return M.fastq(b, q, FC.edge_reads()[2], prefix=prefix, paired=paired)


def last_error():
    return pkg.lib().kc_last_error().decode()


def cpu(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@DEVS
@PACKS
@pytest.mark.parametrize("paired", (False, True), ids=("single", "paired"))
def test_writer_edges(paired, packed, dev):
    o = FC.edge_reads()[2]
    b, q = source(FC.edge_reads(), packed)
    flags = M.PAIRED if paired else 0
    with pkg.KmerCounter(21) as kc:
        for prefix in FC.PREFIXES:
            want = edge_text(packed, paired, prefix)
            for shift, src_shift in ((0, 0), (1, 1), (7, 15), (15, 0), (0, 15), (7, 1)):
                rc, got, w, total = text_call(kc, b, q, o, prefix=prefix, flags=flags, capacity=len(want), dev=dev, shift=shift, src_shift=src_shift)
                assert rc == 0 and (w, total) == (len(want), len(want))
                assert got == want, (prefix, shift, src_shift, next(i for i in range(len(want)) if got[i] != want[i]))
        # the Python side gives the same
        db, dq, do = on(dev, b, q, o)
        assert kc.fastq_text(db, dq, do, paired=paired, check=True) == edge_text(packed, paired, "r")


@PACKS
def test_every_first_byte_with_small_capacities(packed):
    o = FC.small_reads()[2]
    b, q = source(FC.small_reads(), packed)
    want = M.fastq(b, q, o, paired=True, first_id=8)
    assert 64 < len(want) < 100
    with pkg.KmerCounter(21) as kc:
        for dev in (False, True):
            for capacity in (1, 15, 16, 17):
                got = b""
                for first in range(len(want) + 1):
                    rc, piece, w, total = text_call(kc, b, q, o, flags=M.PAIRED, first_id=8, first_byte=first, capacity=capacity, dev=dev,
                                                    shift=first % 16, src_shift=first % 3)
                    assert rc == 0 and total == len(want) and piece == M.window(want, first, capacity), (dev, capacity, first)
                    got += piece[:1]
                assert got == want


@DEVS
@PACKS
def test_windows_of_the_edge_text(packed, dev):
    o = FC.edge_reads()[2]
    b, q = source(FC.edge_reads(), packed)
    want = edge_text(packed, True, "r")
    total = len(want)
    assert total > 16 * 4099
    with pkg.KmerCounter(21) as kc:
        got, first = b"", 0
        while first < total:  # a partition, laid end to end, is the whole
            rc, piece, w, t = text_call(kc, b, q, o, flags=M.PAIRED, first_byte=first, capacity=4099, dev=dev, shift=first % 16, src_shift=1)
            assert rc == 0 and t == total and w == min(4099, total - first)
            got += piece
            first += w
        assert got == want
        for capacity in (4096, 4097, total + 5):
            for first in (1, 4095, 4096, total - 1, total):
                rc, got, w, t = text_call(kc, b, q, o, flags=M.PAIRED, first_byte=first, capacity=capacity, dev=dev, shift=5)
                assert rc == 0 and t == total and got == M.window(want, first, capacity), (capacity, first)
        # behind the end; a size query writes nothing
        rc, _, _, _ = text_call(kc, b, q, o, flags=M.PAIRED, first_byte=total + 1, capacity=16, dev=dev)
        assert rc == E and "kc_fastq_text: first_byte %d is behind the text's %d bytes" % (total + 1, total) in last_error()
        rc, got, w, t = text_call(kc, b, q, o, flags=M.PAIRED, capacity=1 << 20, dev=dev, query=True)
        assert (rc, got, w, t) == (0, b"", 0, total)
        db, dq, do = on(dev, b, q, o)
        assert kc.fastq_text(db, dq, do, paired=True, first_byte=4095, capacity=4097) == want[4095:4095 + 4097]
        for window_bytes in (4099, total + 1):
            out = io.BytesIO()
            assert kc.write_fastq(out, db, dq, do, paired=True, window_bytes=window_bytes) == total and out.getvalue() == want


@DEVS
@PACKS
def test_orders(packed, dev):
    o = FC.edge_reads()[2]
    b, q = source(FC.edge_reads(), packed)
    n = len(o) - 1
    orders = {"reversed": np.arange(n - 1, -1, -1), "subset": np.array([9, 2, 10]), "repeats": np.array([8, 8, 0, 8, 0, 0, 3]),
              "even": np.arange(0, n, 2), "odd": np.arange(1, n, 2), "none": np.zeros(0)}
    with pkg.KmerCounter(21) as kc:
        for name, order in orders.items():
            order = order.astype(np.uint32)
            for flags in (0, M.PAIRED):
                want = M.fastq(b, q, o, order=order, paired=bool(flags), first_id=5)
                rc, got, w, total = text_call(kc, b, q, o, order=order, flags=flags, first_id=5, capacity=len(want) + 3, dev=dev, shift=3, src_shift=1)
                assert rc == 0 and total == len(want) and got == want, (name, flags)
        # no reads at all, with and without an order; PAIRED wants an even count
        none = np.zeros(1, dtype=np.uint64)
        for order in (None, np.zeros(0, dtype=np.uint32)):
            assert text_call(kc, b[:0], q if q is None else q[:0], none, order=order, capacity=16, dev=dev) == (0, b"", 0, 0)
        rc, _, _, _ = text_call(kc, b[:0], q if q is None else q[:0], none, capacity=16, first_byte=1, dev=dev)
        assert rc == E and "first_byte 1 is behind the text's 0 bytes" in last_error()
        assert text_call(kc, b, q, o, flags=M.PAIRED, capacity=64, dev=dev, nreads=n - 1)[0] == E
        assert "kc_fastq_text: KC_FASTQ_OUT_PAIRED with %d reads, an odd number" % (n - 1) in last_error()
        # an entry out of range: the lowest j is named
        bad = np.array([2, 1, n, 0, 0xFFFFFFFF, n + 7], dtype=np.uint32)
        assert text_call(kc, b, q, o, order=bad, capacity=64, dev=dev)[0] == E
        assert "kc_fastq_text: order[2] names no read (%d reads)" % n in last_error()
        assert text_call(kc, b[:0], q if q is None else q[:0], none, order=bad[:1], capacity=64, dev=dev)[0] == E
        assert "kc_fastq_text: order[0] names no read (0 reads)" in last_error()
        # offsets that do not start at 0, that decrease; a read of 2^32 bytes
        for at, value, status in ((0, 1, E), (3, int(o[2]) - 1, E), (n, int(o[n - 1]) + (1 << 32), CAP)):
            off = o.copy()
            off[at] = value
            assert text_call(kc, b, q, off, capacity=64, dev=dev)[0] == status, (at, value)
            assert ("the offsets of %d reads" % n if status == E else "a read of 2^32 bytes or more") in last_error()


@DEVS
def test_numbers_and_their_digits(dev):
    b, q, o = FC.small_reads()
    n = len(o) - 1
    with pkg.KmerCounter(21) as kc:
        for first_id in (7, 8, 97, 98, 999, 10 ** 15 - 2, 10 ** 16 - n):
            for flags in (0, M.PAIRED):
                want = M.fastq(b, q, o, paired=bool(flags), first_id=first_id)
                rc, got, w, total = text_call(kc, b, q, o, flags=flags, first_id=first_id, capacity=len(want), dev=dev, shift=9)
                assert rc == 0 and total == len(want) and got == want, (first_id, flags)
        ids = np.array([9, 10 ** 16 - 1, 10 ** 15, 100], dtype=np.uint64)
        for order in (None, np.array([3, 1, 1, 0, 2], dtype=np.uint32)):
            want = M.fastq(b, q, o, order=order, ids=ids, paired=True, prefix="")
            rc, got, w, total = text_call(kc, b, q, o, order=order, ids=ids, prefix="", flags=M.PAIRED, first_id=77, capacity=len(want), dev=dev, shift=1)
            assert rc == 0 and total == len(want) and got == want
        # seventeen digits are refused, by the lowest j
        assert text_call(kc, b, q, o, first_id=10 ** 16 - n + 1, capacity=64, dev=dev)[0] == E
        assert "kc_fastq_text: the number of record %d has more than 16 digits" % (n - 1) in last_error()
        assert text_call(kc, b, q, o, flags=M.PAIRED, first_id=10 ** 16 - n + 1, capacity=64, dev=dev)[0] == 0  # the pair's first index
        assert text_call(kc, b, q, o, first_id=(1 << 64) - 2, capacity=64, dev=dev)[0] == E and "record 0 has more" in last_error()
        ids[2] = 10 ** 16
        assert text_call(kc, b, q, o, order=np.array([0, 1, 3, 2, 2], dtype=np.uint32), ids=ids, capacity=64, dev=dev)[0] == E
        assert "the number of record 3 has more than 16 digits" in last_error()
        assert text_call(kc, b, q, o, order=np.array([0, 1, 3], dtype=np.uint32), ids=ids, capacity=64, dev=dev)[0] == 0  # left out


def test_positions_over_32_bits():
    b, q, o = FC.reads_of((32767,) * 64, 13, qual_span=32)
    order = (np.arange(70000, dtype=np.uint64) * 37 % 64).astype(np.uint32)
    with pkg.KmerCounter(21) as kc:
        for packed in (False, True):
            sb, sq = (FC.pack(b, q), None) if packed else (b, q)
            for first in ((1 << 32) - 100, None):
                total, _ = M.total_and_window(sb, sq, o, order, 0, 0, paired=True)
                first = total - 50 if first is None else first
                assert total > (1 << 32) + (1 << 28)
                want = M.total_and_window(sb, sq, o, order, first, 4096, paired=True)[1]
                rc, got, w, t = text_call(kc, sb, sq, o, order=order, flags=M.PAIRED, first_byte=first, capacity=4096, dev=True, shift=3)
                assert rc == 0 and t == total and w == len(want) == min(4096, total - first) and got == want, (packed, first)


@DEVS
def test_packed_bytes_of_every_value(dev):
    packed = np.concatenate([np.arange(256), np.arange(255, -1, -1), np.arange(256)[::7]]).astype(np.uint8)
    o = np.array([0, 100, 256, 256, 500, len(packed)], dtype=np.uint64)
    for qual_offset in (33, 64):
        with pkg.KmerCounter(21, qual_offset=qual_offset) as kc:
            want = M.fastq(packed, None, o, qual_offset=qual_offset)
            for src_shift in (0, 1, 15):
                rc, got, w, total = text_call(kc, packed, None, o, capacity=len(want), dev=dev, shift=2, src_shift=src_shift)
                assert rc == 0 and total == len(want) and got == want, (qual_offset, src_shift)
            # with the check the first code over 4 is refused, with its place
            for order in (None, np.array([4, 2, 1, 0], dtype=np.uint32)):
                j, i, which, pos, x = M.first_bad(packed, None, o, order)
                assert text_call(kc, packed, None, o, order=order, flags=M.CHECK, capacity=len(want), dev=dev)[0] == BAD
                assert "kc_fastq_text: record %d (read %d): base %d is 0x%02x, a code over 4" % (j, i, pos, x) in last_error()
            good = np.where((packed & 7) > 4, packed & 0xF8, packed).astype(np.uint8)
            want = M.fastq(good, None, o, qual_offset=qual_offset)
            assert text_call(kc, good, None, o, flags=M.CHECK, capacity=len(want), dev=dev)[1] == want


@DEVS
def test_ascii_check(dev):
    b, q, o = FC.reads_of((40, 1, 0, 33, 16, 200), 14)
    n = len(o) - 1
    want = M.fastq(b, q, o)
    with pkg.KmerCounter(21) as kc:
        assert text_call(kc, b, q, o, flags=M.CHECK, capacity=len(want), dev=dev, src_shift=1)[1] == want
        for x in (0x0A, 0x20, 0x7F, 0x00):
            for read in (0, 1, 3, 5):
                for which in (0, 1):
                    for at in (int(o[read]), int(o[read + 1]) - 1):  # the read's first and last byte
                        arrays = [b.copy(), q.copy()]
                        arrays[which][at] = x
                        hit = M.first_bad(arrays[0], arrays[1], o)
                        assert hit == (read, read, ("base", "quality")[which], at - int(o[read]), x)
                        assert text_call(kc, arrays[0], arrays[1], o, flags=M.CHECK, capacity=len(want), dev=dev, src_shift=at % 3)[0] == BAD
                        assert "kc_fastq_text: record %d (read %d): %s %d is 0x%02x, outside 0x21 .. 0x7e" % hit in last_error()
                        # without the flag the byte is copied as it is
                        assert text_call(kc, arrays[0], arrays[1], o, capacity=len(want), dev=dev)[1] == M.fastq(arrays[0], arrays[1], o)
        # several bad bytes: the first in (j, bases before qualities, position) wins; reads that the order leaves out do not count
        bb, qq = b.copy(), q.copy()
        qq[int(o[0]) + 3] = 0x7F
        bb[int(o[3]) + 30] = 0x20
        bb[int(o[3]) + 2] = 0x0A
        qq[int(o[3])] = 0x00
        bb[int(o[5]) + 199] = 0x80
        for order in (None, [5, 3, 0], [3, 3, 5], [4, 1, 0, 3], [2, 4, 1, 1]):
            order = None if order is None else np.array(order, dtype=np.uint32)
            hit = M.first_bad(bb, qq, o, order)
            rc, got, w, total = text_call(kc, bb, qq, o, order=order, flags=M.CHECK, capacity=len(want), dev=dev)
            if hit is None:
                assert rc == 0 and got == M.fastq(bb, qq, o, order=order)
            else:
                assert rc == BAD and "kc_fastq_text: record %d (read %d): %s %d is 0x%02x, outside" % hit in last_error(), (order, hit)
        assert n == 6


def test_round_trip_of_ascii_pairs_on_the_device():
    b, q, o = FC.reads_of(np.random.default_rng(15).integers(0, 260, size=600), 16)
    db, dq, do = on(True, b, q, o)
    with pkg.KmerCounter(21) as kc:
        text = kc.fastq_text(db, dq, do, paired=True, check=True)
        assert text == M.fastq(b, q, o, paired=True)
        gb, gq, go = kc.fastq_pairs(text)
        assert (cpu(go).view(np.uint64) == o).all() and (cpu(gb) == b).all() and (cpu(gq) == q).all()
        # a pair of files, from host arrays and from device tensors
        for arrays in ((b, q, o), (db, dq, do)):
            f1, f2 = io.BytesIO(), io.BytesIO()
            sizes = kc.write_fastq_pairs(f1, f2, *arrays, window_bytes=50001)
            t1, t2 = f1.getvalue(), f2.getvalue()
            assert sizes == (len(t1), len(t2))
            assert t1 == M.fastq(b, q, o, order=range(0, 600, 2), paired=True) and t2 == M.fastq(b, q, o, order=range(1, 600, 2), paired=True)
        gb, gq, go = kc.fastq_pairs(t1, t2)
        assert (cpu(go).view(np.uint64) == o).all() and (cpu(gb) == b).all() and (cpu(gq) == q).all()
        # a range of pairs
        f1, f2 = io.BytesIO(), io.BytesIO()
        kc.write_fastq_pairs(f1, f2, db, dq, do, first_pair=100, npairs=7, prefix="p")
        assert f1.getvalue() == M.fastq(b, q, o, order=range(200, 214, 2), paired=True, prefix="p")
        assert f2.getvalue() == M.fastq(b, q, o, order=range(201, 214, 2), paired=True, prefix="p")


def test_round_trip_of_merged_reads_and_their_counts():
    import merge_model as MM
    b, q, o = MM.interleave(MM.random_pairs(np.random.default_rng(17), 750, 1, 300) * 2)  # every pair twice: its k-mers are counted
    with pkg.KmerCounter(21) as kc:
        packed, offs, st = kc.merge_pairs(b, q, o)
        n = st["out_reads"]
        assert n > 1500 and st["merged"] > 300
        text = kc.fastq_text(packed, None, offs, check=True)
        assert text == M.fastq(cpu(packed), None, cpu(offs).view(np.uint64))
        p2, o2 = kc.fastq_to_packed(text)
        assert (cpu(o2) == cpu(offs)).all() and (cpu(p2) == cpu(packed)).all()
        kc.submit_packed_reads(p2, o2, nreads=n)
        kc.flush()
        again = kc.sorted_results()
    with pkg.KmerCounter(21) as kc:
        packed, offs, st = kc.merge_pairs(b, q, o)
        kc.submit_packed_reads(packed, offs, nreads=st["out_reads"])
        kc.flush()
        direct = kc.sorted_results()
    assert len(direct[1]) > 1000 and all(np.array_equal(x, y) for x, y in zip(again, direct))


def test_streams_and_the_parts_of_a_shuffle():
    b, q, o = FC.edge_reads()
    want = M.fastq(b, q, o, paired=True, first_id=3)
    with pkg.KmerCounter(21) as kc:
        for dev in (False, True):
            db, dq, do = on(dev, b, q, o)
            assert kc.fastq_text(db, dq, do, paired=True, first_id=3) == want
            for window_bytes in (1, 4099, len(want) + 9):
                if window_bytes == 1:  # byte by byte: a small text
                    sb, sq, so = on(dev, *FC.small_reads())
                    out = io.BytesIO()
                    assert kc.write_fastq(out, sb, sq, so, window_bytes=1) == len(out.getvalue())
                    assert out.getvalue() == M.fastq(*FC.small_reads())
                    continue
                out = io.BytesIO()
                assert kc.write_fastq(out, db, dq, do, paired=True, first_id=3, check=True, window_bytes=window_bytes) == len(want)
                assert out.getvalue() == want
    # shuffle_reads' parts, each to files of its own, parse back to the shuffled arrays
    import links_cases as LC
    from test_gpu_gap_align import block_arrays, read_arrays
    layout, _ = LC.LAYOUTS["gaps"]
    G = LC.genome(19)
    reads, _ = LC.pairs_of(G, 19)
    rb, ro = read_arrays(reads)
    rq = np.random.default_rng(20).integers(35, 74, size=len(rb)).astype(np.uint8)
    with pkg.KmerCounter(LC.K) as kc:
        kc.index_contigs(*block_arrays(LC.contigs_of(G, layout)))
        alns, _, _ = kc.align_reads(rb, ro)
        gapped, _ = kc.align_gapped(rb, ro, alns)
        _, pairs, _ = kc.pair_inserts(ro, gapped, max_insert=1000)
        s = kc.shuffle_reads(rb, rq, ro, gapped, pairs, parts=3)
        starts = [int(x) for x in s["part_starts"]]
        assert len(starts) == 4 and starts[3] == len(reads) // 2
        gb, gq, lens = [], [], []
        for j in range(3):
            f1, f2 = io.BytesIO(), io.BytesIO()
            kc.write_fastq_pairs(f1, f2, s["bases"], s["quals"], s["offsets"], first_pair=starts[j], npairs=starts[j + 1] - starts[j])
            assert f1.getvalue().startswith(b"@r%d/1\n" % (2 * starts[j])) or starts[j] == starts[j + 1]
            pb, pq, po = kc.fastq_pairs(f1.getvalue(), f2.getvalue())
            gb.append(cpu(pb))
            gq.append(cpu(pq))
            lens.append(np.diff(cpu(po)))
        assert (np.concatenate(gb) == cpu(s["bases"])).all() and (np.concatenate(gq) == cpu(s["quals"])).all()
        assert (np.concatenate(lens) == np.diff(cpu(s["offsets"]).astype(np.int64))).all()


def test_scale_200000_reads_in_windows():
    rng = np.random.default_rng(18)
    lens = rng.integers(0, 301, size=200000)
    b, q, o = FC.reads_of(lens, 19)
    # the model, composed per read with numpy: the name lines by Python, the read's two lines as slices
    names = [b"@r%d/%d\n" % (i - (i & 1), 1 + (i & 1)) for i in range(len(lens))]
    bb, qq, oo = b.tobytes(), q.tobytes(), [int(x) for x in o]
    want = b"".join(names[i] + bb[oo[i]:oo[i + 1]] + b"\n+\n" + qq[oo[i]:oo[i + 1]] + b"\n" for i in range(len(lens)))
    assert want[:4096] == M.total_and_window(b, q, o, None, 0, 4096, paired=True)[1]
    db, dq, do = on(True, b, q, o)
    with pkg.KmerCounter(21) as kc:
        out = io.BytesIO()
        assert kc.write_fastq(out, db, dq, do, paired=True, check=True, window_bytes=(1 << 20) + 7) == len(want)
        assert out.getvalue() == want
        packed = FC.pack(b, np.minimum(q, 33 + 31))
        dp, = on(True, packed)
        text = kc.fastq_text(dp, None, do, paired=True)
    bq = np.minimum(q, 33 + 31).tobytes()
    assert text == b"".join(names[i] + bb[oo[i]:oo[i + 1]] + b"\n+\n" + bq[oo[i]:oo[i + 1]] + b"\n" for i in range(len(lens)))


def test_any_state_of_the_context_and_the_kernel_times():
    b, q, o = FC.small_reads()
    want = M.fastq(b, q, o)
    for kw in (dict(), dict(rank_me=1, rank_n=2)):
        with pkg.KmerCounter(21, time_kernels=True, **kw) as kc:
            for step in ("fresh", "submitted", "finalized") if not kw else ("fresh",):
                if step == "submitted":
                    kc.submit_reads(b, q, o)
                elif step == "finalized":
                    kc.finalize()
                kc.kernel_times(clear=True)
                assert kc.fastq_text(b, q, o, order=np.arange(len(o) - 1, dtype=np.uint32), check=True) == want, (kw, step)
                t = {k: v[0] for k, v in kc.kernel_times().items() if "rtext" in k or "<fastq out>" in k}
                assert t == {"kc_rtext_check_kernel": 2, "kc_rtext_bytes_kernel": 1, "kc_rtext_sizes_kernel": 2, "kc_link_tile_scan_kernel<fastq out>": 2,
                             "kc_asm_scan_kernel<fastq out>": 2, "kc_rtext_starts_kernel": 2, "kc_asm_spans_kernel<fastq out>": 1,
                             "kc_rtext_write_kernel": 1}, t
