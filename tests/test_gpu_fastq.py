"""kc_fastq_to_packed_device / kc_fastq_pairs_device against their host twins kc_fastq_to_packed / kc_fastq_pairs:
the same status, counts, output bytes, offsets and kc_last_error() text for well-formed and broken FASTQ, host and
device input; capacity handling; long lines; KC_FASTQ_PARTIAL streaming; a text over 2^32 bytes; the whole stage from
FASTQ text against the host path and the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import merge_model as M
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu
SENT = 0xDEADBEEF  # *nreads / *nbytes before a call: an error leaves them alone
FILL = 0xA5        # output bytes before a call: a failed call writes a prefix, exactly like the host


# ---- one call of each side ------------------------------------------------------------------------------------------
def host_packed(text, qoff, cap=None, rcap=None, arrays=True):
    L = pkg.lib()
    cap = len(text) if cap is None else cap
    rcap = len(text) // 4 + 1 if rcap is None else rcap
    packed = np.full(max(cap, 1), FILL, np.uint8)
    offs = np.full(rcap + 1, SENT, np.uint64)
    n, nb = C.c_uint64(SENT), C.c_uint64(SENT)
    st = L.kc_fastq_to_packed(text, len(text), qoff, packed.ctypes.data if arrays else None, cap, offs.ctypes.data if arrays else None,
                              rcap, C.byref(n), C.byref(nb))
    return st, n.value, nb.value, packed, offs, L.kc_last_error().decode() if st else ""


def dev_packed(kc, text, device_input, cap=None, rcap=None, arrays=True, flags=0):
    import torch
    L = pkg.lib()
    cap = len(text) if cap is None else cap
    rcap = len(text) // 4 + 1 if rcap is None else rcap
    packed = torch.full((max(cap, 1),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.from_numpy(np.full(rcap + 1, SENT, np.uint64).view(np.int64)).cuda()
    n, nb, cons = C.c_uint64(SENT), C.c_uint64(SENT), C.c_uint64(SENT)
    if device_input:
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda() if text else torch.empty(0, dtype=torch.uint8, device="cuda")
        tp = t.data_ptr() if text else None
    else:
        t, tp = text, text
    st = L.kc_fastq_to_packed_device(kc._h, tp, len(text), 1 if device_input else 0, flags, packed.data_ptr() if arrays else None, cap,
                                     offs.data_ptr() if arrays else None, rcap, C.byref(n), C.byref(nb), C.byref(cons))
    err = L.kc_last_error().decode() if st else ""
    return st, n.value, nb.value, packed.cpu().numpy(), offs.cpu().numpy().view(np.uint64), err, cons.value


def host_pairs(t1, t2, cap=None, rcap=None, arrays=True):
    L = pkg.lib()
    tot = len(t1) + (len(t2) if t2 is not None else 0)
    cap = tot if cap is None else cap
    rcap = tot // 4 + 1 if rcap is None else rcap
    b = np.full(max(cap, 1), FILL, np.uint8)
    q = np.full(max(cap, 1), FILL, np.uint8)
    o = np.full(rcap + 1, SENT, np.uint64)
    n, nb = C.c_uint64(SENT), C.c_uint64(SENT)
    st = L.kc_fastq_pairs(t1, len(t1), t2, 0 if t2 is None else len(t2), b.ctypes.data if arrays else None,
                          q.ctypes.data if arrays else None, cap, o.ctypes.data if arrays else None, rcap, C.byref(n), C.byref(nb))
    return st, n.value, nb.value, b, q, o, L.kc_last_error().decode() if st else ""


def _dev_text(t):
    import torch
    if t is None:
        return None, None
    if not t:  # an empty second file is still a second file: any non-NULL address
        e = torch.zeros(1, dtype=torch.uint8, device="cuda")
        return e, e.data_ptr()
    d = torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda()
    return d, d.data_ptr()


def dev_pairs(kc, t1, t2, device_input, cap=None, rcap=None, arrays=True, flags=0):
    import torch
    L = pkg.lib()
    tot = len(t1) + (len(t2) if t2 is not None else 0)
    cap = tot if cap is None else cap
    rcap = tot // 4 + 1 if rcap is None else rcap
    b = torch.full((max(cap, 1),), FILL, dtype=torch.uint8, device="cuda")
    q = torch.full((max(cap, 1),), FILL, dtype=torch.uint8, device="cuda")
    o = torch.from_numpy(np.full(rcap + 1, SENT, np.uint64).view(np.int64)).cuda()
    n, nb, c1, c2 = C.c_uint64(SENT), C.c_uint64(SENT), C.c_uint64(SENT), C.c_uint64(SENT)
    if device_input:
        k1, p1 = _dev_text(t1) if t1 else (None, None)
        k2, p2 = _dev_text(t2)
    else:
        p1, p2 = t1, t2
    st = L.kc_fastq_pairs_device(kc._h, p1, len(t1), p2, 0 if t2 is None else len(t2), 1 if device_input else 0, flags,
                                 b.data_ptr() if arrays else None, q.data_ptr() if arrays else None, cap,
                                 o.data_ptr() if arrays else None, rcap, C.byref(n), C.byref(nb), C.byref(c1), C.byref(c2))
    err = L.kc_last_error().decode() if st else ""
    return (st, n.value, nb.value, b.cpu().numpy(), q.cpu().numpy(), o.cpu().numpy().view(np.uint64), err), (c1.value, c2.value)


def same_packed(kc, text, qoff, device_input, **kw):
    want = host_packed(text, qoff, **kw)
    got = dev_packed(kc, text, device_input, **kw)[:6]
    ctx = (text[:300], device_input, kw)
    assert got[0] == want[0], (got[5], want[5], ctx)
    assert got[5] == want[5], ctx
    assert got[1:3] == want[1:3], ctx
    assert np.array_equal(got[3], want[3]), ctx
    assert np.array_equal(got[4], want[4]), ctx
    return want


def same_pairs(kc, t1, t2, device_input, **kw):
    want = host_pairs(t1, t2, **kw)
    got = dev_pairs(kc, t1, t2, device_input, **kw)[0]
    ctx = (t1[:200], None if t2 is None else t2[:200], device_input, kw)
    assert got[0] == want[0], (got[6], want[6], ctx)
    assert got[6] == want[6], ctx
    assert got[1:3] == want[1:3], ctx
    for i in (3, 4, 5):
        assert np.array_equal(got[i], want[i]), (i, ctx)
    return want


# ---- generated FASTQ ------------------------------------------------------------------------------------------------
GOOD = b"ACGTacgtNn"
IUPAC = b"URYKMSWBDHV"
BAD = b"XEZuryj.-*0 \x00\xff\x80@+"


def make_records(rng, n, max_len=40, name_len=(1, 12)):
    recs = []
    for _ in range(n):
        ln = int(rng.integers(0, max_len + 1))
        alpha = GOOD + (IUPAC if rng.random() < 0.3 else b"")
        seq = bytes(rng.choice(np.frombuffer(alpha, np.uint8), ln).tolist())
        qual = bytes(rng.integers(33, 127, ln).astype(np.uint8).tolist())
        name = b"@" + bytes(rng.integers(33, 127, int(rng.integers(*name_len))).astype(np.uint8).tolist())
        plus = b"+" + (name[1:] if rng.random() < 0.2 else b"")
        recs.append([name, seq, plus, qual])
    return recs


def render(rng, recs, style=None):
    out = []
    for r in recs:
        for line in r:
            s = style if style is not None else rng.integers(0, 4)
            end = (b"\n", b"\r\n", b" \t\r\n", b"\t \n")[s]
            out.append(line + end)
    return b"".join(out)


def mutate(rng, recs):
    """one of the broken or odd shapes, on the record list (before rendering) or on the text (after)"""
    kind = int(rng.integers(0, 14))
    n = len(recs)
    i = int(rng.integers(0, n)) if n else 0
    post = None
    if n and kind == 0:
        recs[i][0] = recs[i][0][1:] if rng.random() < 0.5 else b"X" + recs[i][0]
    elif n and kind == 1:
        recs[i][2] = b"" if rng.random() < 0.3 else b"-" + recs[i][2]
    elif n and kind == 2:
        recs[i][3] = recs[i][3] + b"I" if rng.random() < 0.5 else recs[i][3][:-1]
    elif n and kind in (3, 4) and recs[i][1]:
        s = bytearray(recs[i][1])
        s[0 if kind == 3 else len(s) - 1] = int(rng.choice(np.frombuffer(BAD, np.uint8)))
        recs[i][1] = bytes(s)
    elif n > 1 and kind == 5:  # a structural error with a bad base before or after it
        j = int(rng.integers(0, n))
        if recs[j][1]:
            s = bytearray(recs[j][1])
            s[int(rng.integers(0, len(s)))] = ord("X")
            recs[j][1] = bytes(s)
        recs[i][0] = b"name"
    elif kind == 6:
        post = ("cut", None)
    elif kind == 7:
        post = ("tail", b"\n" * int(rng.integers(1, 4)))
    elif kind == 8:
        post = ("noeol", None)
    elif kind == 9:
        post = ("blank", None)
    elif n and kind == 10:  # a name line of white space only
        recs[i][0] = b" \t"
    elif n and kind == 11:  # two bad bases: the first wins
        s = bytearray(recs[i][1] + b"AAAA")
        s[1], s[3] = ord("Z"), ord("E")
        recs[i][1] = bytes(s)
        recs[i][3] = recs[i][3] + b"IIII"
    return post


def finish(rng, text, post):
    if post is None:
        return text
    if post[0] == "cut":
        return text[: int(rng.integers(0, len(text) + 1))]
    if post[0] == "tail":
        return text + post[1]
    if post[0] == "noeol":
        return text.rstrip(b"\n")
    # an empty line after a random line
    ends = [i for i, c in enumerate(text) if c == 10]
    if not ends:
        return text
    at = ends[int(rng.integers(0, len(ends)))] + 1
    return text[:at] + b"\n" + text[at:]


def gen_text(rng, nrec=None, max_len=40):
    n = int(rng.integers(0, 8)) if nrec is None else nrec
    recs = make_records(rng, n, max_len)
    post = mutate(rng, recs) if rng.random() < 0.7 else None
    return finish(rng, render(rng, recs, style=None if rng.random() < 0.5 else 0), post)


# ---- the tests ------------------------------------------------------------------------------------------------------
HAND = [
    b"", b"\n", b"\n\n", b"@r\nACGT\n+\nIIII", b"@r\nACGT\n+\nIIII\n", b"@r\nACGT\n+\nIIII\n\n", b"@r\nACGT\n+\nIIII\n\n\n",
    b"@r\nACGT\n+\nIIII\n\n\n\n", b"@r\nACGT\n+\nIII\n", b"r\nACGT\n+\nIIII\n", b"@r\nACGT\n-\nIIII\n", b"@r\nACGT\n+\n",
    b"@r\nACGT\n", b"@r\n", b"@r", b"@r\r\nAC GT\r\n+\r\nIIIII\r\n", b"@r\nAXGT\n+\nIIII\n", b"@r\nACGX\n+\nIIII\n",
    b"@r\nacgtnNURYKMSWBDHV\n+\n" + b"!" * 17 + b"\n", b"@r\nryk\n+\nIII\n", b"@r\nACGT \t\r\n+ \nIIII\r\n", b" \n",
    b"@r\n\n+\n\n", b"@r\n\n+\n\n@s\nA\n+\n~\n", b"@a\nAC\n+\nII\n\n@b\nAC\n+\nII\n", b"@a\nAC\n+\n\n", b"@\nA\n+\nI\n \t\r",
]


@pytest.mark.parametrize("qoff", [33, 64])
def test_packed_hand_cases(qoff):
    with pkg.KmerCounter(21, qual_offset=qoff) as kc:
        for t in HAND:
            for dev in (False, True):
                same_packed(kc, t, qoff, dev)


def test_pairs_hand_cases():
    with pkg.KmerCounter(21) as kc:
        for t in HAND:
            for dev in (False, True):
                same_pairs(kc, t, None, dev)
                same_pairs(kc, t, HAND[4], dev)
                same_pairs(kc, HAND[4], t, dev)


@pytest.mark.parametrize("qoff", [33, 64])
def test_packed_fuzz(qoff):
    rng = np.random.default_rng(7 + qoff)
    with pkg.KmerCounter(21, qual_offset=qoff) as kc:
        for it in range(1500):
            same_packed(kc, gen_text(rng), qoff, bool(it & 1))


def test_pairs_fuzz():
    rng = np.random.default_rng(11)
    with pkg.KmerCounter(21) as kc:
        for it in range(1500):
            dev = bool(it & 1)
            if it % 3 == 0:  # interleaved, odd counts included
                same_pairs(kc, gen_text(rng), None, dev)
                continue
            n1 = int(rng.integers(0, 6))
            n2 = n1 if rng.random() < 0.5 else int(rng.integers(0, 6))  # unequal counts in both directions
            t1 = gen_text(rng, n1) if rng.random() < 0.5 else render(rng, make_records(rng, n1))
            t2 = gen_text(rng, n2) if rng.random() < 0.5 else render(rng, make_records(rng, n2))
            same_pairs(kc, t1, t2, dev)


def test_capacity_and_size_query():
    rng = np.random.default_rng(3)
    with pkg.KmerCounter(21) as kc:
        for it in range(200):
            recs = make_records(rng, int(rng.integers(1, 6)))
            text = good = render(rng, recs)
            st, nr, nb = host_packed(text, 33)[:3]
            assert st == _lib.KC_OK
            if it % 4 == 3:  # an error after records that fit: the error wins
                text += b"@bad\nAXC\n+\nIII\n"
                st = _lib.KC_ERR_BAD_BASE
            dev = bool(it & 1)
            same_packed(kc, text, 33, dev, arrays=False)
            for cap, rcap in ((0, 0), (max(nb - 1, 0), nr), (nb, max(nr - 1, 0)), (nb, nr), (nb // 2, nr // 2)):
                w = same_packed(kc, text, 33, dev, cap=cap, rcap=rcap)
                if st == _lib.KC_OK and (cap < nb or rcap < nr):
                    assert w[0] == _lib.KC_ERR_CAPACITY and w[1:3] == (nr, nb)
            t2 = render(rng, make_records(rng, len(recs)))
            nr, nb = host_pairs(good, t2)[1:3]
            same_pairs(kc, text, t2, dev, arrays=False)
            for cap, rcap in ((0, 0), (max(nb - 1, 0), nr), (nb, max(nr - 1, 0)), (nb, nr)):
                same_pairs(kc, text, t2, dev, cap=cap, rcap=rcap)


def test_long_lines():
    rng = np.random.default_rng(5)
    recs = [[b"@mega", bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 1 << 20).tolist()), b"+", b"I" * (1 << 20)]]
    for _ in range(6):
        recs.append([b"@" + b"h" * 10000, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100000).tolist()), b"+" + b"h" * 10000,
                     bytes(rng.integers(33, 127, 100000).astype(np.uint8).tolist())])
    recs += make_records(rng, 50, 200)
    text = render(rng, recs, style=0)
    with pkg.KmerCounter(21) as kc:
        w = same_packed(kc, text, 33, True)
        assert w[0] == _lib.KC_OK and w[1] == len(recs)
        same_packed(kc, text, 33, False)
        same_pairs(kc, text[: text.rfind(b"@")], None, True)  # drops one record: an odd, then an even count
        same_pairs(kc, text, None, True)
        # a bad base deep inside the long read, and one after it in a 100 kb read
        bad = bytearray(text)
        bad[len(b"@mega\n") + 777777] = ord("X")
        bad[text.index(b"+" + b"h" * 10) - 5] = ord("Z")
        same_packed(kc, bytes(bad), 33, True)
        same_pairs(kc, bytes(bad), None, True)


def _whole_end(text, records):
    """byte past the last of `records` whole records (4 lines ending in '\\n' each)"""
    if records == 0:
        return 0
    pos = -1
    for _ in range(4 * records):
        pos = text.index(b"\n", pos + 1)
    return pos + 1


def _stream(kc, text, cuts, device_input, pairs=False):
    """feed text in blocks ending at `cuts`, carrying the tail; returns the concatenated outputs and the last status"""
    outs, offs, tail, base = [], [np.zeros(1, np.uint64)], b"", 0
    bounds = list(cuts) + [len(text)]
    prev = 0
    for i, b in enumerate(bounds):
        buf = tail + text[prev:b]
        prev = b
        last = i == len(bounds) - 1
        flags = 0 if last else _lib.KC_FASTQ_PARTIAL
        if pairs:
            (st, nr, nb, bb, qq, oo, err), (cons, _) = dev_pairs(kc, buf, None, device_input, flags=flags)
            data = (bb[:nb] if st == 0 else None, qq[:nb] if st == 0 else None)
        else:
            st, nr, nb, pk, oo, err, cons = dev_packed(kc, buf, device_input, flags=flags)
            data = (pk[:nb] if st == 0 else None,)
        if st:
            return st, err, None, None
        if not last:
            whole = buf.count(b"\n") // 4
            if pairs:
                whole &= ~1
            assert cons == _whole_end(buf, whole)
        outs.append(data)
        offs.append(oo[1:nr + 1] + base)
        base += nb
        tail = buf[cons:] if not last else b""
    cat = tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))
    return 0, "", cat, np.concatenate(offs)


def test_partial_streaming():
    rng = np.random.default_rng(9)
    with pkg.KmerCounter(21) as kc:
        for it in range(60):
            text = render(rng, make_records(rng, int(rng.integers(0, 40)), 120), style=None if it % 2 else 0)
            if it % 5 == 4:
                text += b"\n"
            cuts = sorted(rng.integers(0, len(text) + 1, int(rng.integers(0, 8))).tolist())
            for pairs in (False, True):
                if pairs:
                    want = host_pairs(text, None)
                    w = (want[0], want[1], want[2], (want[3][: want[2]], want[4][: want[2]]), want[5][: want[1] + 1], want[6])
                else:
                    want = host_packed(text, 33)
                    w = (want[0], want[1], want[2], (want[3][: want[2]],), want[4][: want[1] + 1], want[5])
                st, err, cat, offs = _stream(kc, text, cuts, bool(it & 1), pairs)
                assert st == w[0], (it, pairs, err, w[5])  # (an error's text counts from the start of its block)
                if st == 0:
                    assert np.array_equal(offs, w[4])
                    for a, b in zip(cat, w[3]):
                        assert np.array_equal(a, b)
        # a malformed unfinished record in the tail is no error until the last call
        good = render(rng, make_records(rng, 10), style=0)
        text = good + b"@broken\nACGT\n-\n"
        st, nr, nb, pk, oo, err, cons = dev_packed(kc, text, True, flags=_lib.KC_FASTQ_PARTIAL)
        assert st == 0 and nr == 10 and cons == len(good)
        assert np.array_equal(pk[:nb], host_packed(good, 33)[3][:nb])
        want = host_packed(text, 33)
        got = dev_packed(kc, text, True)
        assert want[0] == got[0] == _lib.KC_ERR_INVALID_ARG and want[5] == got[5]
        # two files stream up to the same record count
        t1 = render(rng, make_records(rng, 7), style=0)
        t2 = render(rng, make_records(rng, 5), style=0) + b"@half\nAC"
        (st, nr, nb, *_), (c1, c2) = dev_pairs(kc, t1, t2, True, flags=_lib.KC_FASTQ_PARTIAL)
        assert st == 0 and nr == 10 and c1 == _whole_end(t1, 5) and c2 == _whole_end(t2, 5)
        same_pairs(kc, t1[:c1], t2[:c2], True)


def test_text_over_4_gib():
    import torch
    rng = np.random.default_rng(1)
    block = render(rng, [[b"@read%04d" % i, bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 150).tolist()), b"+",
                          bytes(rng.integers(33, 80, 150).astype(np.uint8).tolist())] for i in range(1024)], style=0)
    st, nr0, nb0, pk0, of0, _ = host_packed(block, 33)
    assert st == 0 and nr0 == 1024
    reps = (1 << 32) // len(block) + 2
    with pkg.KmerCounter(21) as kc:
        text = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda().repeat(reps)
        assert text.numel() > 1 << 32
        packed, offs = kc.fastq_to_packed(text)
        del text
        n = reps * 1024
        assert offs.numel() == n + 1 and packed.numel() == reps * nb0
        assert int(offs[-1].item()) == reps * nb0
        for r in (0, 1023, 1024, n // 2 + 17, n - 1):
            rep, j = divmod(r, 1024)
            o = int(offs[r].item())
            assert o == rep * nb0 + int(of0[j])
            ln = int(of0[j + 1] - of0[j])
            assert np.array_equal(packed[o:o + ln].cpu().numpy(), pk0[int(of0[j]):int(of0[j]) + ln])


def test_record_sums_scan_one_item_into_second_round():
    """2 097 153 records are 8 193 workgroups of 256 output records: the single-workgroup scan of their sequence sums
    takes 8 192 items a round, so it carries into a second round of exactly one item.  About 60 MB of text, made and
    compared on the device."""
    import torch
    block = b"@frontend_scan_rec_1\nA\n+\nI\n@frontend_scan_rec_2\nCG\n+\n5I\n@frontend_scan_rec_3\nTNa\n+\nI!I\n"
    st, nr0, nb0, pk0, of0, _ = host_packed(block, 33)
    assert st == 0 and nr0 == 3 and list(of0[:4]) == [0, 1, 3, 6]
    reps = 699051
    n = 3 * reps
    assert n == 2097153 and (n + 255) // 256 == 8193
    with pkg.KmerCounter(21) as kc:
        text = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda().repeat(reps)
        packed, offs = kc.fastq_to_packed(text)
        del text
        assert offs.numel() - 1 == n  # nreads
        want = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        want[1:] = torch.cumsum(torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda").repeat(reps), 0)
        assert int(want[-1].item()) == 4194306 and int(offs[-1].item()) == 4194306
        assert torch.equal(offs, want)
        assert torch.equal(packed, torch.from_numpy(pk0[:nb0].copy()).cuda().repeat(reps))


def _reads_text(rng, nreads, k_genome=4000):
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), k_genome)
    recs = []
    for i in range(nreads):
        ln = int(rng.integers(60, 151))
        st = int(rng.integers(0, k_genome - ln))
        s = genome[st:st + ln].copy()
        for p in rng.integers(0, ln, rng.poisson(0.5)):
            s[p] = ord("N")
        recs.append([b"@r%d/%d" % (i // 2, 1 + i % 2), s.tobytes(), b"+", rng.choice([35, 45, 73], ln).astype(np.uint8).tobytes()])
    return recs


@pytest.mark.parametrize("k", [21, 33, 77])
def test_stage_from_fastq_matches_host_path_and_oracle(k, tmp_path):
    from oracle import cpu_oracle as O
    rng = np.random.default_rng(200 + k)
    text = render(rng, _reads_text(rng, 3000), style=0)
    (gk, gc, gl, gr), st = pkg.analyze_kmers_fastq(k, 33, text)
    hp, ho = pkg.fastq_to_packed(text)
    with pkg.KmerCounter(k) as kc:
        kc.submit_packed_reads(hp, ho)
        kc.flush()
        hk, hc, hl, hr = kc.sorted_results()
        hst = kc.stats()
    assert gk.shape == hk.shape and (gk == hk).all() and (gc == hc).all() and (gl == hl).all() and (gr == hr).all()
    assert {s: st[s] for s in ("num_reads", "raw_kmers", "num_unique")} == {s: hst[s] for s in ("num_reads", "raw_kmers", "num_unique")}
    ab, aq, ao = M.packed_to_ascii(hp, ho)
    orc = O.Oracle(k, nranks=1, nthreads=2)
    orc.add_reads(ab, aq, ao)
    ok, oc, ol, orr = orc.finalize()
    assert gk.shape == ok.shape and (gk == ok).all() and (gc == oc).all() and (gl == ol).all() and (gr == orr).all()
    assert st["raw_kmers"] == orc.stats()["raw_kmers"]
    # streamed from a file in small blocks
    path = tmp_path / "reads.fq"
    path.write_bytes(text)
    with pkg.KmerCounter(k) as kc:
        assert kc.submit_fastq(str(path), block_bytes=4099) == 3000
        kc.flush()
        sk, sc, sl, sr = kc.sorted_results()
    assert sk.shape == gk.shape and (sk == gk).all() and (sc == gc).all() and (sl == gl).all() and (sr == gr).all()


@pytest.mark.parametrize("k", [21, 33, 77])
def test_paired_stage_from_fastq_matches_host_path_and_oracle(k):
    from oracle import cpu_oracle as O
    rng = np.random.default_rng(300 + k)
    recs = _reads_text(rng, 2000)
    t1 = render(rng, recs[0::2], style=0)
    t2 = render(rng, recs[1::2], style=1)
    (gk, gc, gl, gr), st, mst = pkg.analyze_kmers_fastq_paired(k, 33, t1, t2)
    b, q, o = pkg.fastq_pairs(t1, t2)
    (hk, hc, hl, hr), hst, hmst = pkg.analyze_kmers_paired(k, 33, b, q, o)
    assert mst == hmst
    assert gk.shape == hk.shape and (gk == hk).all() and (gc == hc).all() and (gl == hl).all() and (gr == hr).all()
    (ik, ic, il, ir), _, imst = pkg.analyze_kmers_fastq_paired(k, 33, render(rng, recs, style=0))
    assert imst == mst and ik.shape == gk.shape and (ik == gk).all() and (ic == gc).all()
    packed, offs, want = M.merge_pairs(b, q, o, 33, k)
    ab, aq, ao = M.packed_to_ascii(packed, offs)
    orc = O.Oracle(k, nranks=1, nthreads=2)
    orc.add_reads(ab, aq, ao)
    ok, oc, ol, orr = orc.finalize()
    assert gk.shape == ok.shape and (gk == ok).all() and (gc == oc).all() and (gl == ol).all() and (gr == orr).all()


def test_python_wrappers_accept_every_text_form():
    import torch
    rng = np.random.default_rng(4)
    text = render(rng, make_records(rng, 30, 80), style=0)
    hp, ho = pkg.fastq_to_packed(text)
    with pkg.KmerCounter(21) as kc:
        for t in (text, np.frombuffer(text, np.uint8), torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()):
            p, o = kc.fastq_to_packed(t)
            assert np.array_equal(p.cpu().numpy(), hp) and np.array_equal(o.cpu().numpy().view(np.uint64), ho)
        hb, hq, hpo = pkg.fastq_pairs(text)
        b, q, o = kc.fastq_pairs(text)
        assert np.array_equal(b.cpu().numpy(), hb) and np.array_equal(q.cpu().numpy(), hq)
        assert np.array_equal(o.cpu().numpy().view(np.uint64), hpo)
        with pytest.raises(_lib.KcError):
            kc.fastq_to_packed(text + b"@x\nAC\n+\nI\n")
