"""kc_ctg_dedup (csrc/kc_dedup.hpp) against the host model tests/dedup_model.py, byte for byte: the records, the block, its
offsets, the depths and all sixteen words of the statistics, from host arrays and from device tensors.  The model is never
replaced by a second device run.

Every call goes through `call`: the outputs are slices of larger poisoned arrays, the block and the depths at a chosen
offset, and everything outside what the call may write must stay poisoned."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import dedup_cases as DC
import dedup_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

POISON = 0xA5
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
BOTH = pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))


def on(dev, *arrays):
    """the arrays as they are, or as device tensors (unsigned integers as the signed ones: the bits)"""
    if not dev:
        return arrays
    import torch
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(SIGNED.get(a.dtype, a.dtype)).copy()).cuda() for a in arrays)


def addr(a):
    return None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def host(a, dtype):
    return a.cpu().numpy().view(dtype) if hasattr(a, "data_ptr") else a


def call(kc, seqs, offsets, depths, dev, capacity=None, query=False, shift=0, with_recs=True, **kw):
    """One raw call.  -> dict(rc, n, nbytes, stats, seqs, offsets, depths, records); the poison around the outputs is checked
    here, and on an error that nothing at all was written (KC_ERR_CAPACITY for the block: nothing but the totals)."""
    import torch
    n = len(offsets) - 1
    cap = len(seqs) if capacity is None else capacity
    s, o, d = on(dev, seqs, offsets, depths)
    room = shift + cap + 64
    out_s, out_d = np.full(room, POISON, dtype=np.uint8), np.full(room, 0xA5A5, dtype=np.uint16)
    out_o, out_r = np.full(n + 5, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(32 * (n + 2), POISON, dtype=np.uint8)
    out_s, out_d, out_o, out_r = on(dev, out_s, out_d, out_o, out_r)
    prm = _lib.kc_dedup_params(kw.get("max_mismatches", 0), 1 if kw.get("duplicates_only") else 0, kw.get("max_candidates", 0))
    st, nk, nb = _lib.kc_dedup_stats(contigs=77, longest_removed=77), C.c_uint64(77), C.c_uint64(77)
    torch.cuda.synchronize()
    rc = pkg.lib().kc_ctg_dedup(kc._h, addr(s) if len(seqs) else None, len(seqs), addr(o), n, addr(d), 1 if dev else 0, C.byref(prm),
                                addr(out_r) if with_recs else None, None if query else addr(out_s) + shift, cap, addr(out_o),
                                None if depths is None else addr(out_d) + 2 * shift, C.byref(nk), C.byref(nb), C.byref(st))
    got_s, got_d, got_o, got_r = host(out_s, np.uint8), host(out_d, np.uint16), host(out_o, np.uint64), host(out_r, np.uint8)
    k, total = int(nk.value), int(nb.value)
    wrote = rc == _lib.KC_OK and not query
    if not wrote:
        assert (got_s == POISON).all() and (got_d == 0xA5A5).all() and (got_o == 0xA5A5A5A5A5A5A5A5).all() and (got_r == POISON).all()
    told = rc == _lib.KC_OK or (rc == _lib.KC_ERR_CAPACITY and total != 77)
    if not told:
        assert (k, total, st.contigs, st.longest_removed) == (77, 77, 77, 77)
        return dict(rc=rc)
    assert list(st.reserved) == [0, 0]
    out = dict(rc=rc, n=k, nbytes=total, stats=pkg.kcount._stats_dict(st))
    if wrote:
        assert total <= cap and (got_s[:shift] == POISON).all() and (got_s[shift + total:] == POISON).all()
        assert (got_o[k + 1:] == 0xA5A5A5A5A5A5A5A5).all() and (got_r[32 * n if with_recs else 0:] == POISON).all()
        assert (got_d[:shift] == 0xA5A5).all() and (got_d[shift + (total if depths is not None else 0):] == 0xA5A5).all()
        out.update(seqs=got_s[shift:shift + total].copy(), offsets=got_o[:k + 1].copy(), records=got_r[:32 * n].copy(),
                   depths=None if depths is None else got_d[shift:shift + total].copy())
    return out


def random_depths(seqs, seed=5):
    d = np.random.default_rng(seed).integers(1, 65536, len(seqs)).astype(np.uint16)
    d[seqs == ord("_")] = 0
    return d


def model_of(ctgs, k, depths_flat=None, **kw):
    """the model on a block's contigs, the depths given per byte of the input block"""
    per = None
    if depths_flat is not None:
        _, offsets = M.block(ctgs)
        per = [depths_flat[int(offsets[u]):int(offsets[u]) + len(c)] for u, c in enumerate(ctgs)]
    return M.dedup(ctgs, k, depths=per, **kw)


def same(got, want, where):
    """the device's outputs are the model's, byte for byte"""
    assert got["rc"] == 0, (where, pkg.lib().kc_last_error())
    assert list(got["stats"]) == list(M.STATS) and got["stats"] == want["stats"], (where, got["stats"], want["stats"])
    assert (got["n"], got["nbytes"]) == (len(want["ctgs"]), len(want["seqs"])), where
    if "seqs" not in got:
        return
    recs = got["records"].view(M.REC_DTYPE)
    for f in M.REC_DTYPE.names:
        assert (recs[f] == want["records"][f]).all(), (where, f, np.flatnonzero(np.atleast_1d((recs[f] != want["records"][f]).reshape(len(recs), -1).any(1)))[:5])
    assert got["records"].tobytes() == want["records"].tobytes(), where
    assert got["seqs"].tobytes() == want["seqs"].tobytes(), where
    assert (got["offsets"] == want["offsets"]).all(), where
    if want["depths"] is not None and got["depths"] is not None:
        assert (got["depths"] == want["depths"]).all(), where


def check(kc, ctgs, k, dev, shift=0, with_depths=True, want=None, **kw):
    ctgs = M.as_bytes(ctgs)
    seqs, offsets = M.block(ctgs)
    depths = random_depths(seqs) if with_depths else None
    want = want or model_of(ctgs, k, depths, **kw)
    got = call(kc, seqs, offsets, depths, dev, shift=shift, **kw)
    same(got, want, (k, dev, kw))
    return got, want


@BOTH
@pytest.mark.parametrize("k", DC.KS)
def test_hand_cases(k, dev):
    with pkg.KmerCounter(k) as kc:
        for i, (name, ctgs, kw, removed) in enumerate(DC.cases(k)):
            got, want = check(kc, ctgs, k, dev, shift=i % 16, with_depths=i % 2 == 0, **kw)
            recs = got["records"].view(M.REC_DTYPE)
            assert {u for u in range(len(ctgs)) if recs["status"][u] != M.KEPT} == set(removed), (k, name)


# ---- a single mismatch at the chunk boundaries of the comparison, at every alignment of either side -------------------
K = 21
SPOTS = (0, 15, 16, 17, 1023, 1024, 2999)  # bytes of the 3 000-base contig; 2999 is the last


@functools.lru_cache(maxsize=None)
def spots_block():
    """For every alignment of the container's side (16), spot (7) and strand (2) a container and its 3 000-base contig,
    whose start runs through the 16 alignments as well: 224 pairs, every relative shift of the two sides among them.  The
    differing byte is an N in the contig, so that its anchor -- the first all-ACGT window -- still matches exactly."""
    r = random.Random(11)
    ctgs, planted = [], []
    at = 0  # the block position of the next contig

    def add(t):
        nonlocal at
        ctgs.append(bytes(t))
        at += len(t) + 1
        return len(ctgs) - 1

    i = 0
    for dst in range(16):
        for spot in SPOTS:
            for o in (0, 1):
                u_text = bytearray(r.choice(b"ACGT") for _ in range(3000))
                head, tail = bytes(r.choice(b"ACGT") for _ in range(32)), bytes(r.choice(b"ACGT") for _ in range(20 + i % 7))
                # the container's compared bytes start at block position `at + pad + 32`: pad makes that = dst mod 16
                pad = (dst - (at + 1 + 32)) % 16
                add(b"N" * pad)  # at + 1 counted its separator; now at % 16 == (dst - 32) % 16
                v = add(head + bytes(u_text) + tail)
                assert (at - len(ctgs[v]) - 1 + 32) % 16 == dst
                u_text[spot] = ord("N")
                src = (dst + 1 + i) % 16  # the contig's own start: every alignment, every difference to dst
                add(b"N" * ((src - (at + 1)) % 16))
                u = add(M.rc(bytes(u_text)) if o else bytes(u_text))
                assert (at - 3001) % 16 == src
                planted.append((u, v, o))
                i += 1
    return ctgs, planted


@functools.lru_cache(maxsize=None)
def spots_model(mm):
    return M.dedup(spots_block()[0], K, max_mismatches=mm)


@BOTH
@pytest.mark.parametrize("mm", (0, 1))
def test_one_mismatch_at_every_chunk_boundary_and_alignment(mm, dev):
    ctgs, planted = spots_block()
    want = spots_model(mm)
    for u, v, o in planted:  # by construction
        r = want["records"][u]
        assert (r["status"], r["container"], r["pos"], r["orient"], r["mismatches"]) == ((M.CONTAINED, v, 32, o, 1) if mm else (M.KEPT, M.NONE, 0, 0, 0))
    with pkg.KmerCounter(K) as kc:
        check(kc, ctgs, K, dev, want=want, with_depths=False, max_mismatches=mm)


@BOTH
def test_three_mismatches_leave_early(dev):
    r = random.Random(12)
    a = bytes(r.choice(b"ACGT") for _ in range(9000))
    b = bytearray(a[40:40 + 8000])
    for p in (100, 101, 7000):  # two in one chunk: the wave is over the limit of 2 only behind the third
        b[p] = ord("N")
    c = bytearray(a[:5000])
    c[30], c[31], c[32] = b"NNN"  # over the limit in the first step
    with pkg.KmerCounter(K) as kc:
        for mm, gone in ((2, 0), (3, 2)):
            for flip in (False, True):
                ctgs = [a, M.rc(bytes(b)) if flip else bytes(b), M.rc(bytes(c)) if flip else bytes(c)]
                got, want = check(kc, ctgs, K, dev, max_mismatches=mm)
                assert want["stats"]["contained"] == gone and want["stats"]["candidates"] == 2


@functools.lru_cache(maxsize=None)
def long_pair():
    r = random.Random(13)
    a = bytearray(r.choice(b"ACGT") for _ in range(300000))
    b = bytearray(a)
    b[-1] = ord("A") if a[-1] != ord("A") else ord("C")
    return [bytes(a), bytes(b), M.rc(bytes(b))]


@functools.lru_cache(maxsize=None)
def long_model(mm):
    return M.dedup(long_pair(), K, max_mismatches=mm)


@BOTH
@pytest.mark.parametrize("mm", (0, 1))
def test_a_long_pair_that_differs_in_its_last_byte(mm, dev):
    """300 000 bases, far over the 16 KiB at which a candidate is cut into segments of 8 KiB, a wave each"""
    want = long_model(mm)
    st = want["stats"]
    # contig 1 against contig 0 differs in the last byte.  Contig 2 = rc(contig 1) is an exact duplicate of it at either
    # limit, and its anchor holds the differing byte, so contig 0 is no candidate for it: with one mismatch allowed its
    # named container is itself redundant, as the header says it may be
    assert (st["kept"], st["duplicates"], st["candidates"]) == ((1, 2, 2) if mm else (2, 1, 2))
    assert want["records"]["mismatches"][1] == mm and want["records"]["container"][2] == 1
    with pkg.KmerCounter(K) as kc:
        check(kc, long_pair(), K, dev, shift=3, want=want, with_depths=dev, max_mismatches=mm)


# ---- many short contigs -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_block():
    """About 2 000 contigs of 21 .. 5 000 bases: disjoint pieces of a random genome with N runs and a repeat, and a tenth as
    many planted copies -- whole or a slice, flipped or not, with 0 .. 4 changed bases.  -> (contigs, exact, lonely): the
    indices of the exact copies that must go, and of the pieces that overlap nothing and must stay."""
    r = random.Random(14)
    g = bytearray(r.choice(b"ACGT") for _ in range(1900000))
    g[900000:903000] = g[100000:103000]  # a repeat
    for _ in range(60):
        p = r.randrange(len(g))
        n = min(r.randrange(1, 80), len(g) - p)
        g[p:p + n] = b"N" * n
    pieces, p = [], 0
    while p + 5100 < len(g):
        n = int(21 * (5000 / 21) ** r.random())
        pieces.append((p, n))
        p += n + r.randrange(1, 30)
    items = [("piece", bytes(g[p:p + n]), (p, n)) for p, n in pieces]
    for _ in range(len(pieces) // 10):
        p, n = r.choice(pieces)
        t = bytes(g[p:p + n])
        whole = r.random() < 0.3 or n < 2 * K
        if not whole:
            a = r.randrange(n - K)
            t = t[a:a + r.randrange(K, n - a + 1)]
        changed = r.choice((0, 0, 1, 2, 4))
        t = bytearray(t)
        for _ in range(changed):
            q = r.randrange(len(t))
            t[q] = ord("A") if t[q] != ord("A") else ord("G")
        t = bytes(t)
        items.append(("exact" if changed == 0 and len(t) < n else "copy", M.rc(t) if r.random() < 0.5 else t, (p, n)))
    r.shuffle(items)
    ctgs = [t for _, t, _ in items]
    in_repeat = lambda p, n: p < 103000 and p + n > 100000 or p < 903000 and p + n > 900000  # noqa: E731
    copied = {src for kind, _, src in items if kind != "piece"}
    exact = [u for u, (kind, t, _) in enumerate(items) if kind == "exact" and M.windows(t, K)]
    lonely = [u for u, (kind, _, src) in enumerate(items) if kind == "piece" and src not in copied and not in_repeat(*src)]
    return ctgs, exact, lonely


@functools.lru_cache(maxsize=None)
def many_model(mm, dup_only):
    ctgs = many_block()[0]
    return model_of(ctgs, K, random_depths(M.block(ctgs)[0]), max_mismatches=mm, duplicates_only=dup_only)


@BOTH
@pytest.mark.parametrize("mm,dup_only", ((0, False), (1, False), (3, False), (0, True)))
def test_many_short_contigs(mm, dup_only, dev):
    ctgs, exact, lonely = many_block()
    assert 1800 < len(ctgs) < 2600 and len(exact) >= 40 and len(lonely) > 1000
    want = many_model(mm, dup_only)
    status = want["records"]["status"]
    if mm == 0 and not dup_only:  # the ground truth by construction
        assert (status[exact] == M.CONTAINED).all() and (status[lonely] == M.KEPT).all()
    assert want["stats"]["contained"] + want["stats"]["duplicates"] > (0 if dup_only else len(exact))
    with pkg.KmerCounter(K) as kc:
        check(kc, ctgs, K, dev, shift=9, want=want, max_mismatches=mm, duplicates_only=dup_only)


# ---- compaction ---------------------------------------------------------------------------------------------------------
@BOTH
def test_compaction_edges(dev):
    r = random.Random(15)
    rnd = lambda n: bytes(r.choice(b"ACGT") for _ in range(n))  # noqa: E731
    a, b, c = rnd(700), rnd(333), rnd(90)
    blocks = {"first and last removed": [a[5:300], b, a, c, M.rc(b[7:200])],
              "all but one removed": [a[:100], a, M.rc(a), a[600:], a[1:], a],
              "nothing removed": [a, b, c, b"", rnd(20), b"NNNN", rnd(21)],
              "one contig": [c],
              "chunks over many contigs": [rnd(1 + i % 5) for i in range(100)] + [rnd(40), b"", b""]}
    with pkg.KmerCounter(K) as kc:
        for name, ctgs in blocks.items():
            for with_depths in (True, False):
                for shift in (0, 1, 8, 15):
                    got, want = check(kc, ctgs, K, dev, shift=shift, with_depths=with_depths)
            kept = want["stats"]["kept"]
            if name == "first and last removed":
                assert want["kept"] == [1, 2, 3] and len(want["seqs"]) % 16 != 0
            if name == "all but one removed":
                assert want["kept"] == [1] and want["records"]["absorbed"][1] == 5
            if name in ("nothing removed", "one contig", "chunks over many contigs"):
                seqs, offsets = M.block(ctgs)
                assert kept == len(ctgs) and got["seqs"].tobytes() == seqs.tobytes() and (got["offsets"] == offsets).all()
                assert (call(kc, seqs, offsets, random_depths(seqs), dev)["depths"] == random_depths(seqs)).all()


# ---- protocol -----------------------------------------------------------------------------------------------------------
@BOTH
def test_protocol(dev):
    L = pkg.lib()
    name, ctgs, kw, _ = DC.cases(K)[5]
    seqs, offsets = M.block(ctgs)
    depths = random_depths(seqs)
    want = model_of(ctgs, K, depths)
    total = len(want["seqs"])
    assert 0 < total < len(seqs)
    with pkg.KmerCounter(K) as kc:
        # a size query: the totals and the statistics, nothing else
        got = call(kc, seqs, offsets, depths, dev, query=True)
        same(got, want, "query")
        assert "seqs" not in got
        # exactly the capacity; twice the same call gives the same bytes; without records
        first = call(kc, seqs, offsets, depths, dev, capacity=total, shift=5)
        same(first, want, "exact")
        again = call(kc, seqs, offsets, depths, dev, capacity=total, shift=5)
        assert all(first[f].tobytes() == again[f].tobytes() for f in ("seqs", "offsets", "depths", "records")) and first["stats"] == again["stats"]
        bare = call(kc, seqs, offsets, None, dev, with_recs=False)
        assert bare["rc"] == 0 and bare["seqs"].tobytes() == want["seqs"].tobytes() and bare["depths"] is None
        # one byte short
        short = call(kc, seqs, offsets, depths, dev, capacity=total - 1)
        assert short["rc"] == _lib.KC_ERR_CAPACITY and (short["n"], short["nbytes"], short["stats"]) == (len(want["ctgs"]), total, want["stats"])
        assert b"kc_ctg_dedup: %d bytes, the array holds %d" % (total, total - 1) in L.kc_last_error()
        # one candidate too many: both numbers, nothing written, no truncation
        cands = want["stats"]["candidates"]
        assert cands > 1
        over = call(kc, seqs, offsets, depths, dev, max_candidates=cands - 1)
        assert over == dict(rc=_lib.KC_ERR_CAPACITY) and b"kc_ctg_dedup: %d candidates, max_candidates is %d" % (cands, cands - 1) in L.kc_last_error()
        same(call(kc, seqs, offsets, depths, dev, max_candidates=cands), want, "at the limit")
        # no contigs
        none = call(kc, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), None, dev)
        assert (none["rc"], none["n"], none["nbytes"]) == (0, 0, 0) and list(none["offsets"]) == [0] and not any(none["stats"].values())
        # a bad byte, bad offsets: refused, and `call` saw that nothing was written
        low = seqs.copy()
        low[3] = ord("a")
        assert call(kc, low, offsets, depths, dev) == dict(rc=_lib.KC_ERR_BAD_BASE) and b"kc_ctg_dedup: a byte outside ACGTN" in L.kc_last_error()
        for at, value in ((0, 1), (1, int(offsets[1]) - 1), (2, int(offsets[1])), (len(offsets) - 1, len(seqs) - 1), (1, 1 << 40)):
            bad = offsets.copy()
            bad[at] = value
            assert call(kc, seqs, bad, depths, dev) == dict(rc=_lib.KC_ERR_INVALID_ARG), (at, value)
            assert b"kc_ctg_dedup: the offsets of %d contigs" % len(ctgs) in L.kc_last_error()
        if dev:
            import torch
            t = torch.zeros(64, dtype=torch.uint8, device="cuda")
            s, o = on(True, seqs, offsets)
            p, nk, nb = _lib.kc_dedup_params(), C.c_uint64(0), C.c_uint64(0)
            torch.cuda.synchronize()
            rc = L.kc_ctg_dedup(kc._h, addr(s), len(seqs), addr(o), len(ctgs), None, 1, C.byref(p), addr(t) + 8, None, 0, None, None, C.byref(nk),
                                C.byref(nb), None)
            assert rc == _lib.KC_ERR_INVALID_ARG and b"kc_ctg_dedup: a device record array is 16-byte aligned" in L.kc_last_error()


def test_host_arrays_and_device_tensors_give_the_same_and_the_wrapper_returns_them():
    name, ctgs, kw, _ = DC.cases(K)[5]
    seqs, offsets = M.block(ctgs)
    depths = random_depths(seqs)
    want = model_of(ctgs, K, depths)
    with pkg.KmerCounter(K, time_kernels=True) as kc:
        h, d = call(kc, seqs, offsets, depths, False), call(kc, seqs, offsets, depths, True)
        assert all(h[f].tobytes() == d[f].tobytes() for f in ("seqs", "offsets", "depths", "records")) and h["stats"] == d["stats"]
        for dev in (False, True):
            s, o, dp = on(dev, seqs, offsets, depths)
            out = kc.dedup_contigs(s, o, dp)
            assert len(out) == 5 and (hasattr(out[0], "is_cuda") and out[0].is_cuda) == dev
            got = [host(out[0], np.uint8), host(out[1], np.uint64), host(out[2], np.uint16), host(out[3], np.uint8)]
            assert got[0].tobytes() == want["seqs"].tobytes() and (got[1] == want["offsets"]).all() and (got[2] == want["depths"]).all()
            assert got[3].tobytes() == want["records"].tobytes() and out[4] == want["stats"]
            assert kc.dedup_contigs(s, o)[2] is None
            assert [t.encode() for t in kc.dedup_strings(s, o)] == want["ctgs"]
            assert kc.dedup_strings(s, o, duplicates_only=True) == [t.decode() for t in model_of(ctgs, K, duplicates_only=True)["ctgs"]]
        with pytest.raises(pkg.KcError, match="candidates, max_candidates is 1"):
            kc.dedup_contigs(seqs, offsets, max_candidates=1)
        with pytest.raises(ValueError, match="depths"):
            kc.dedup_contigs(seqs, offsets, depths[:-1])
        names = set(kc.kernel_times())
        assert {"kc_dedup_anchor_kernel", "kc_dedup_windows_kernel<count>", "kc_dedup_verify_kernel", "kc_dedup_gather_kernel<depths>",
                "kc_align_check_kernel<dedup>"} <= names, names
