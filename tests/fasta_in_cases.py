"""Seeded builders of FASTA texts for the tests of kc_fasta_to_block, and the one way its GPU tests call the library: every
output array a slice of a larger poisoned array at a chosen byte offset, of exactly the capacity, the poison around it
checked."""
import ctypes as C
import functools

import numpy as np

import fasta_in_model as M

POISON = 0xA5
LINE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)
# headers and what the rules make of them: (id, depth or None, flags), None where the default depth stands
HEADERS = ((b">Contig0 17.4", 0, 17, 3), (b">noid", 0, None, 0), (b">x123456789012345678 12.5", 123456789012345678, 13, 3),
           (b">x1234567890123456789 12.49", 0, 12, 2), (b">big_7\t70000", 7, 65535, 3), (b">sci_8 1e3", 8, None, 1), (b">dot_9  12.", 9, 12, 3),
           (b">ten_10 1234567890", 10, None, 1), (b">" + b"k" * 250 + b"_42 33", 42, None, 1), (b">" + b"j" * 300 + b"_5 9", 0, None, 0),
           (b">9", 9, None, 1), (b"> 5 6", 0, 5, 2), (b">" + b"m" * 251 + b"_7", 7, None, 1), (b">" + b"m" * 252 + b"_7 1", 7, None, 1),
           (b">" + b"m" * 253 + b"_7 1", 0, None, 0),
           (b">scaffold_17 trailing words 3", 17, None, 1), (b">a1 999999999.96", 1, 65535, 3), (b">a2 0.5 ", 2, 1, 3))


def bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


@functools.lru_cache(maxsize=None)
def edge_text(last="header", seed=7):
    """One text with every edge of the rules (see tests/test_gpu_fasta_in.py); it ends in an unterminated header, or with
    last="bases" in an unterminated sequence line."""
    rng = np.random.default_rng(seed)
    t = [b"\n", b" \t\r\n", b">lines\n"] + [bases(rng, n) + b"\n" for n in LINE_LENGTHS]
    t += [b">crlf_1\r\n", bases(rng, 40) + b"\r\n", b"\r\n", bases(rng, 7) + b" \t\r\n", bases(rng, 16) + b"  \n"]
    t += [b">e%d\n" % i for i in range(5)] + [b"\n"]
    for i in range(24):  # several separators in one 16-byte chunk
        t += [b">s%d\n" % i, bases(rng, 1 + i % 3) + b"\n"] if i % 5 else [b">s%d\n" % i]
    t += [b">table 3\n", M.ACCEPTED + b"\n", M.ACCEPTED[::-1] * 3 + b"\r\n"]
    for h, _, _, _ in HEADERS:
        t += [h + b"\n", bases(rng, int(rng.integers(0, 40))) + b"\n"]
    t += [b">long\n", bases(rng, 200000) + b"\n", b">wrapped 8\n"] + [bases(rng, 60) + b"\n" for _ in range(100)] + [bases(rng, 13) + b"\n"]
    t += [b">last_99 4"] if last == "header" else [b">last_99 4\n", bases(rng, 20)]
    return b"".join(t)


def small_text():
    """about 400 bytes with every kind of line, for the cut at every byte; a bad byte near its end"""
    rng = np.random.default_rng(11)
    t = [b"\n>a_1 3.5\n", bases(rng, 33) + b"\n", bases(rng, 16) + b"\r\n", b">b\n>c_2\t7\n", b"acgtnRY\n", b"\n", b">d\r\n", bases(rng, 70) + b"\n"]
    t += [b">e_5 1\n", bases(rng, 15) + b"\n", bases(rng, 17) + b"\n", b">f 2\n", bases(rng, 31) + b"  \n", b">g\n", bases(rng, 32) + b"\n" + bases(rng, 60) + b"\n"]
    t += [b">h_9 12.5\n", b"ACGTXACGT\n", b">i\n", bases(rng, 20)]
    return b"".join(t)


def wrap(seq, width):
    return seq + b"\n" if not width or not seq else b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def composed(seed, n, max_len, width):
    """n contigs of 0 .. max_len bases as one text and its expected block, composed without the model's loop over bytes:
    -> (text, seqs, offsets, ids, depths per record).  Contig j has the header ">c_j d" with d = j % 70000."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, max_len + 1, size=n)
    lengths[rng.random(n) < 0.05] = 0
    all_bases = bases(rng, int(lengths.sum()))
    parts, block, at = [], [], 0
    for j, l in enumerate(lengths):
        s = all_bases[at:at + l]
        at += l
        parts.append(b">c_%d %d\n" % (j, j % 70000))
        parts.append(wrap(s, width))
        block.append(s)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths + 1)
    seqs = np.frombuffer(b"_".join(block) + b"_", dtype=np.uint8)
    return b"".join(parts), seqs, offsets, lengths


def on_device(a):
    import torch
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
    return torch.from_numpy(np.ascontiguousarray(a).view(signed.get(a.dtype, a.dtype)).copy()).cuda()


def addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def call(kc, text, flags=0, default_depth=0, dev=False, text_shift=0, shift=0, seqs_capacity=0, ctgs_capacity=0, depths=True, records=True, query=False):
    """kc_fasta_to_block on `text` laid text_shift bytes into a buffer; seqs begins `shift` bytes into a poisoned array, depths
    `shift` entries, offsets and records one entry.  -> dict(status, error, n_ctgs, nbytes, consumed, stats, and the arrays
    up to what the call reported).  On an error every array and every counter must be as it was."""
    import torch
    import mhm2_kmer_analysis_v2_amd as pkg
    from mhm2_kmer_analysis_v2_amd import _lib, kcount
    L = pkg.lib()
    buf = np.full(text_shift + len(text) + 16, POISON, dtype=np.uint8)
    buf[text_shift:text_shift + len(text)] = np.frombuffer(text, dtype=np.uint8)
    room = {"seqs": (np.uint8, shift + seqs_capacity + 64, shift), "offsets": (np.uint64, ctgs_capacity + 1 + 9, 1),
            "depths": (np.uint16, shift + seqs_capacity + 64, shift), "records": (np.uint64, 4 * (ctgs_capacity + 9), 4)}
    arrays = {k: np.full(n, POISON * 0x0101010101010101 & (2 ** (8 * np.dtype(t).itemsize) - 1), dtype=t) for k, (t, n, _) in room.items()}
    if dev:
        buf = on_device(buf)
        arrays = {k: on_device(v) for k, v in arrays.items()}
    at = {k: addr(arrays[k]) + room[k][2] * np.dtype(room[k][0]).itemsize for k in arrays}
    prm = _lib.kc_fasta_in_params(flags, default_depth)
    nc, nb, cons, st = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77), _lib.kc_fasta_in_stats(lines=77, with_depth=77)
    torch.cuda.synchronize()
    rc = L.kc_fasta_to_block(kc._h, addr(buf) + text_shift if len(text) else None, len(text), 1 if dev else 0, C.byref(prm), None if query else at["seqs"],
                             seqs_capacity, None if query else at["offsets"], ctgs_capacity, at["depths"] if depths else None,
                             at["records"] if records else None, C.byref(nc), C.byref(nb), C.byref(cons), C.byref(st))
    got = {k: (v.cpu().numpy().view(room[k][0]) if dev else v) for k, v in arrays.items()}
    out = dict(status=rc, error=L.kc_last_error().decode() if rc else None, n_ctgs=int(nc.value), nbytes=int(nb.value), consumed=int(cons.value))
    poison = {k: got[k].view(np.uint8) == POISON for k in got}
    if rc not in (_lib.KC_OK, _lib.KC_ERR_CAPACITY):
        assert all(p.all() for p in poison.values()) and (nc.value, nb.value, cons.value, st.lines, st.with_depth) == (77, 77, 77, 77, 77)
        return out
    out["stats"] = kcount._stats_dict(st)
    assert list(st.reserved) == [0] * 6
    if rc == _lib.KC_ERR_CAPACITY or query:
        assert all(p.all() for p in poison.values())
        return out
    c, b = out["n_ctgs"], out["nbytes"]
    used = {"seqs": b, "offsets": c + 1, "depths": b if depths else 0, "records": 4 * c if records else 0}
    for k, (t, n, first) in room.items():
        size = np.dtype(t).itemsize
        assert poison[k][:first * size].all() and poison[k][(first + used[k]) * size:].all(), k
        out[k] = got[k][first:first + used[k]]
    out["records"] = out["records"].view(M.REC_DTYPE) if records else None
    out["depths"] = out["depths"] if depths else None
    return out


def same(got, want, depths=True, records=True):
    """the call's result against the model's, field by field"""
    assert got["status"] == want["status"] and got["error"] == want["error"], (got["status"], got["error"], want["error"])
    if want["status"]:  # nothing is written on an error, `consumed` neither
        return
    assert got["consumed"] == want["consumed"]
    assert (got["n_ctgs"], got["nbytes"]) == (len(want["offsets"]) - 1, len(want["seqs"]))
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    if "seqs" not in got:
        return
    bad = np.flatnonzero(got["seqs"] != want["seqs"])
    assert not len(bad), ("seqs", int(bad[0]), len(bad))
    assert (got["offsets"] == want["offsets"]).all()
    if depths:
        assert (got["depths"] == want["depths"]).all()
    if records:
        assert got["records"].tobytes() == want["records"].tobytes(), [(j, g, w) for j, (g, w) in enumerate(zip(got["records"], want["records"])) if g != w][:3]
