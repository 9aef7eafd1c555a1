"""Seeded builders of reads for the tests of kc_fastq_text, and the one way its GPU tests call the library: the window is a
slice of a poisoned array at a byte shift, the source arrays begin at a byte shift of their allocation, and the poison in
front of and behind the window is checked."""
import ctypes as C
import functools

import numpy as np

POISON = 0xA5
EDGE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 150, 151, 32767, 0, 16, 1, 0)
PREFIXES = ("", "r", "a-32-byte-prefix-for-the-records")
assert len(PREFIXES[2]) == 32


def reads_of(lengths, seed, qual_span=94):
    """ASCII reads of these lengths: bases of ACGTN, qualities '!' + [0, qual_span) -> (bases, quals, offsets)"""
    rng = np.random.default_rng(seed)
    offsets = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    n = int(offsets[-1])
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=n, p=(0.24, 0.24, 0.24, 0.24, 0.04))]
    quals = (33 + rng.integers(0, qual_span, size=n)).astype(np.uint8)
    return np.ascontiguousarray(bases), quals, offsets


def pack(bases, quals, qual_offset=33):
    """the read cache's bytes of ASCII reads: code | min(quality, 31) << 3"""
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    q = np.minimum(quals.astype(np.int64) - qual_offset, 31).astype(np.uint8)
    return (code[bases] | (q << 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def edge_reads():
    """an even number of reads of every length at which the writer takes another path, in one block; qualities that a
    packed byte holds"""
    return reads_of(EDGE_LENGTHS + (33,), 11, qual_span=32)


@functools.lru_cache(maxsize=None)
def small_reads():
    return reads_of((3, 0, 17, 1), 12, qual_span=32)


def on(dev, *arrays):
    """the arrays as they are, or as device tensors (uint64 as int64, uint32 as int32: the bits)"""
    if not dev:
        return arrays
    import torch
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(signed.get(a.dtype, a.dtype)).copy()).cuda() for a in arrays)


def addr(a):
    return None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def shifted(dev, a, shift):
    """a copy of the byte array that begins `shift` bytes into an allocation of exactly shift + len bytes -> (keep-alive, address)"""
    if a is None:
        return None, None
    room = np.full(max(shift + len(a), 1), POISON, dtype=np.uint8)  # an empty array has no address
    room[shift:shift + len(a)] = a
    room, = on(dev, room)
    return room, addr(room) + shift


def text_call(kc, bases, quals, offsets, order=None, ids=None, prefix="r", flags=0, first_id=0, first_byte=0, capacity=0, dev=False, shift=0,
              src_shift=0, query=False, nreads=None):
    """-> (status, the window's bytes, written, total); quals None: packed.  The poison around the window is checked here."""
    import torch
    import mhm2_kmer_analysis_v2_amd as pkg
    from mhm2_kmer_analysis_v2_amd import _lib
    n = len(offsets) - 1 if nreads is None else nreads
    n_order = n if order is None else len(order)
    keep_b, pb = shifted(dev, bases, src_shift)
    keep_q, pq = shifted(dev, quals, src_shift)
    padded = None if order is None else np.append(np.asarray(order, dtype=np.uint32), np.uint32(0xFFFFFFFF))  # an address for no entries too
    o, od, idd = on(dev, offsets, padded, ids)
    prefix = prefix.encode() if isinstance(prefix, str) else prefix
    prm = _lib.kc_fastq_out_params(flags | (_lib.KC_FASTQ_OUT_PACKED if quals is None else 0), len(prefix), first_id, prefix)
    room = shift + capacity + 64
    buf = torch.full((room,), POISON, dtype=torch.uint8, device="cuda") if dev else np.full(room, POISON, dtype=np.uint8)
    written, total = C.c_uint64(77), C.c_uint64(77)
    torch.cuda.synchronize()
    rc = pkg.lib().kc_fastq_text(kc._h, pb if len(bases) else None, pq, addr(o), n, addr(od), n_order,
                                 addr(idd), 1 if dev else 0, C.byref(prm), first_byte, None if query else addr(buf) + shift, capacity,
                                 C.byref(written), C.byref(total))
    got = buf.cpu().numpy() if dev else buf
    w = int(written.value)
    if rc != _lib.KC_OK:
        assert (got == POISON).all() and (w, total.value) == (77, 77)
        return rc, b"", w, int(total.value)
    assert w <= capacity and (got[:shift] == POISON).all() and (got[shift + w:] == POISON).all()
    del keep_b, keep_q
    return rc, got[shift:shift + w].tobytes(), w, int(total.value)
