"""Python host side over the C ABI: mirrors the reference's analyze_kmers flow.

  reference (src/kcount/kcount.cpp:142-161)          here
  -------------------------------------------        --------------------------------
  FastqReader + PackedRead (fastq.cpp:1028-1140)    .fastq_to_packed(...)    kc_fastq_to_packed_device
  Adapters ctor + load_adapter_seqs (adapters.cpp)   .load_adapters(...)      kc_adapters_load
  Adapters::trim_pair / trim (adapters.cpp:171-273)  .trim_adapters(...)      kc_trim_adapters
  merge_reads' pair loop (merge_reads.cpp:469-648)   .merge_pairs(...)        kc_merge_pairs
  merge_reads' --dump-merged (merge_reads.cpp:635)   .write_fastq(...)        kc_fastq_text
  KmerDHT ctor -> HashTableInserter::init             KmerCounter(k, ...)      kc_create
  count_kmers: per read quality-mask + process_seq    .submit_reads(...)       kc_submit_reads
  kmer_dht->flush_updates()                           .flush()                 kc_flush
  kmer_dht->finish_updates()                          .finalize()              kc_finalize
  local_kmers (KmerMap)                               .results()               kc_copy_results
  dump_kmers ("KMER count L R", kmer_dht.cpp:284)     .dump_lines()            (host)
                                                      .sort_results()          kc_sort_results
                                                      .dump_text(...)          kc_dump_text_device
  (traverse_debruijn_graph: commented out there)      .unitigs()               kc_build_unitigs
  (no counterpart: duplicate / contained contigs)     .dedup_contigs(...)      kc_ctg_dedup
  get_kmer_count over a sequence's k-mers             .kmer_depths(...)        kc_seq_kmer_depths
  (no counterpart: the histogram of the counts)       .count_spectrum()        kc_count_spectrum
  (ctgs.print_stats: commented out there)             .select_contigs(...)     kc_ctg_select
  (ctgs.dump_contigs: commented out there)            .write_fasta(...)        kc_fasta_text
  (options.ctgs_fname / --checkpoint: likewise)       .load_contigs(...)       kc_fasta_to_block
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (check, kc_align_stats, kc_aln_scores, kc_config, kc_ctg_index_stats, kc_depth_stats, kc_gap_stats, kc_insert_stats, kc_kernel_time, kc_lassm_params, kc_lassm_stats, kc_link_params, kc_link_stats, kc_merge_stats, kc_result, kc_stats, kc_synth_params, kc_trim_stats, kc_tuning,
                   kc_unitig_stats, lib)


def _ptr(a):
    """numpy array / torch tensor / int / None -> address, and whether it is device memory."""
    if a is None:
        return None, False
    if isinstance(a, int):
        return a, True
    if hasattr(a, "data_ptr"):  # torch tensor
        return a.data_ptr(), bool(a.is_cuda)
    return a.ctypes.data, False


def _reads(bases, quals, offsets, nreads=None):
    """The reads of a call -> the addresses of bases, quals (None: none) and offsets, the number of reads (by default
    what the offsets hold) and whether bases is device memory."""
    pb, dev = _ptr(bases)
    n = (len(offsets) - 1) if nreads is None else nreads
    return pb, _ptr(quals)[0], _ptr(offsets)[0], n, dev


def _span(offsets, n):
    """the bytes of the first n reads, from host or device offsets"""
    return int(offsets[n]) - int(offsets[0]) if n else 0


def _records(name, a, dtype, contiguous=True, required=False):
    """A record array argument -> (address, or None where there are no records; number of records; on the device).
    Device records come as a uint8 tensor of count * itemsize bytes; a host array is checked for the item size and for
    being contiguous (contiguous=False: only the item size).  required: the library wants the array even where it is
    empty, so it is checked and its address passed as it is."""
    p, dev = _ptr(a)
    n = a.numel() // dtype.itemsize if dev else len(a)
    if not dev and (n or required) and (a.dtype.itemsize != dtype.itemsize or (contiguous and not a.flags["C_CONTIGUOUS"])):
        raise ValueError("%s: a contiguous array of %d-byte records" % (name, dtype.itemsize))
    return (p if n or required else None), n, dev


def _side(ref, dev, **others):
    """Which side a call is on: that of its argument `ref`, which is on the device or not (dev).  others: name =
    (on the device, number of elements) of every other array; one that has elements lies on the same side.  The error
    names the fewer: the arrays that are not where most of the call's are, or all of them where it is a draw."""
    sides = {True: [], False: []}
    sides[bool(dev)].append(ref)
    for name, (d, n) in others.items():
        if n:
            sides[bool(d)].append(name)
    if sides[True] and sides[False]:
        few, many = sorted(sides.items(), key=lambda kv: len(kv[1]))
        if len(few[1]) == len(many[1]):
            raise ValueError("%s: not on one side; a call's arrays are all host arrays or all device tensors" % ", ".join(few[1] + many[1]))
        raise ValueError("%s: %s among %s; a call's arrays are all host arrays or all device tensors" % (
            ", ".join(few[1]), "on the device" if few[0] else "in host memory", "host arrays" if few[0] else "device tensors"))
    return dev


# torch has no unsigned 16-, 32- and 64-bit integers: the signed ones hold the bits
_TORCH_OF = {"uint8": "uint8", "uint16": "int16", "uint32": "int32", "uint64": "int64"}


def _debug_fill():
    """The byte of KC_DEBUG_FILL as the library reads it (csrc/kc_debug_fill.hpp: decimal or 0x.., 0..255, nothing else), or
    None: what outputs nobody asked zeroed are made of, so that an element the library did not write shows."""
    s = os.environ.get("KC_DEBUG_FILL", "")
    hexa = s[:2] in ("0x", "0X")
    digits = s[2:] if hexa else s
    allowed = "0123456789abcdefABCDEF" if hexa else "0123456789"
    if not digits or any(ch not in allowed for ch in digits):
        return None
    v = int(digits, 16 if hexa else 10)
    return v if v <= 255 else None


class _Out:
    """One output array of a call, of n elements of a record dtype or a scalar dtype, and its address (ptr).  device None:
    a numpy array of zeros; else the torch device: an uninitialised tensor (zeroed=True: zeros), records as uint8 bytes of
    n * itemsize.  With KC_DEBUG_FILL set, either is made of that byte unless zeroed=True asks for zeros.  pad: room for
    one element where n is 0, so that the library gets an address; an exact array of no elements has torch's address 0 on
    the device, which the library reads as NULL -- for the seqs of a call, a size query."""

    def __init__(self, device, n, dtype, pad=False, zeroed=False):
        dtype = np.dtype(dtype)
        # elements of `a` to one of the n: the bytes of a record on the device, else one
        self.n, self.size = n, dtype.itemsize if dtype.fields and device is not None else 1
        m = max(n, 1) if pad else n
        fill = None if zeroed else _debug_fill()
        if device is None:
            self.a = np.zeros(m, dtype=dtype)
            if fill is not None:
                self.a.view(np.uint8)[...] = fill
        else:
            import torch
            kind = torch.uint8 if dtype.fields else getattr(torch, _TORCH_OF[dtype.name])
            self.a = (torch.zeros if zeroed else torch.empty)(m * self.size, dtype=kind, device=device)
            if fill is not None:
                self.a.view(torch.uint8).fill_(fill)
        self.ptr = _ptr(self.a)[0]

    def first(self, n=None):
        """the first n elements (by default the n it was made for)"""
        return self.a[:(self.n if n is None else n) * self.size]


def _stats_dict(st):
    """A statistics struct as a dict: integers, lists of integers for array fields, nothing of `reserved`."""
    values = ((f, getattr(st, f)) for f, _ in st._fields_ if f != "reserved")
    return {f: [int(x) for x in v] if isinstance(v, C.Array) else int(v) for f, v in values}


def _retry_on_capacity(capacity, call, below=None):
    """call(capacity) allocates that much, calls the library and returns (status, the size the library reported, the
    array).  Where the guess was too small -- KC_ERR_CAPACITY and a larger size reported (and one below `below`) -- the
    call is made once more with that size, never a third time."""
    rc, told, out = call(capacity)
    if rc == _lib.KC_ERR_CAPACITY and capacity < told and (below is None or told < below):
        rc, told, out = call(told)  # the size it was told
    return rc, told, out


def _block_strings(seqs, offsets):
    """A seq block (every sequence followed by '_') and its starts, host arrays or device tensors, as Python strings."""
    if not isinstance(seqs, np.ndarray):
        seqs, offsets = seqs.cpu().numpy(), offsets.cpu().numpy()
    text = seqs.tobytes().decode()
    return [text[int(offsets[i]):int(offsets[i + 1]) - 1] for i in range(len(offsets) - 1)]


def _adapter_counts(fn, *args):
    """the loader's four counters, which kc_adapters_load and kc_adapters_index return behind their other arguments"""
    v = [C.c_uint64(0) for _ in range(4)]
    check(getattr(lib(), fn)(*args, *[C.byref(x) for x in v]), fn)
    return dict(zip(("n_adapters", "n_short", "n_entries", "n_kmers"), (x.value for x in v)))


def _text_on_device(t):
    return hasattr(t, "data_ptr") and bool(t.is_cuda)


def _text(t):
    """FASTQ text -> (address, length, on_device, keep-alive): bytes-like and numpy uint8 arrays are host memory, a
    uint8 torch tensor on the GPU is read in place."""
    if hasattr(t, "data_ptr"):
        if t.dtype.itemsize != 1 or not t.is_contiguous():
            raise ValueError("FASTQ text tensors must be contiguous uint8")
        if not t.is_cuda:
            a = t.numpy()
            return (a.ctypes.data if a.size else None), a.size, False, a
        return t.data_ptr(), t.numel(), True, t
    if isinstance(t, str):
        t = t.encode()
    a = np.ascontiguousarray(t if isinstance(t, np.ndarray) else np.frombuffer(t, dtype=np.uint8))
    if a.dtype != np.uint8:
        raise ValueError("FASTQ text arrays must be uint8")
    return (a.ctypes.data if a.size else None), a.size, False, a


class _DeviceWords:
    """Raw device memory of the library as something torch can view without a copy (__cuda_array_interface__)."""

    def __init__(self, ptr, nwords, device):
        self.__cuda_array_interface__ = {"shape": (nwords,), "typestr": "<i8", "data": (ptr, False), "version": 2}
        self.device = device

    def tensor(self):
        import torch
        return torch.as_tensor(self, device=self.device)


def synth_params(**kw):
    p = kc_synth_params()
    lib().kc_synth_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown synth parameter %r" % k)
        setattr(p, k, v)
    return p


def synth_reads_host(nreads, first_read=0, params=None):
    """Host generator (same bytes as the device generator): bases u8, quals u8, offsets u64."""
    p = params or synth_params()
    L = p.read_len
    bases = np.empty(nreads * L, dtype=np.uint8)
    quals = np.empty(nreads * L, dtype=np.uint8)
    offs = np.empty(nreads + 1, dtype=np.uint64)
    check(lib().kc_synth_reads_host(C.byref(p), first_read, nreads, bases.ctypes.data, quals.ctypes.data, offs.ctypes.data),
          "kc_synth_reads_host")
    return bases, quals, offs


class KmerCounter:
    """One shard (one GPU) of the k-mer analysis stage."""

    def __init__(self, kmer_len, qual_offset=33, dmin_thres=2, device=0, rank_me=0, rank_n=1, max_elems=0, time_kernels=False,
                 max_kmers_buffered=0, tuning=None, reference_owner=False, shard_buckets=False, wire_units=False):
        L = lib()
        cfg = kc_config(kmer_len=kmer_len, qual_offset=qual_offset, dmin_thres=dmin_thres, device=device, rank_me=rank_me,
                        rank_n=rank_n, max_elems=max_elems, flags=(_lib.KC_FLAG_TIME_KERNELS if time_kernels else 0) | (_lib.KC_FLAG_REFERENCE_OWNER if reference_owner else 0) | (_lib.KC_FLAG_SHARD_BUCKETS if shard_buckets else 0) | (_lib.KC_FLAG_WIRE_UNITS if wire_units else 0),
                        reserved=0,
                        max_kmers_buffered=max_kmers_buffered)
        st = C.c_int(0)
        self._h = L.kc_create(C.byref(cfg), C.byref(st))
        if not self._h:
            raise _lib.KcError(st.value, "kc_create")
        self._wire_units = bool(wire_units)
        self.k = kmer_len
        self.nl = L.kc_num_longs(kmer_len)          # words of a k-mer in results, dumps and lookups (the reference's)
        self.rec_nl = L.kc_record_longs(kmer_len)   # words of a record on the shard wire (extract_partition / insert_records)
        self.rank_me, self.rank_n = rank_me, rank_n
        self.device = device
        self._tuning = tuning
        if tuning:
            self.set_tuning(**tuning)

    def set_tuning(self, **kw):
        """Geometry overrides of the bucketed path (tests / tuning): mode, writers, p1, p2, slots,
        chunk1, chunk2, chain1_max, chain2_max, arena1, ovf_capacity."""
        t = kc_tuning()
        for k, v in kw.items():
            if not hasattr(t, k):
                raise TypeError("unknown tuning field %r" % k)
            setattr(t, k, v)
        check(lib().kc_set_tuning(self._h, C.byref(t)), "kc_set_tuning")

    def close(self):
        if getattr(self, "_h", None):
            lib().kc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_handle):
        check(lib().kc_set_stream(self._h, stream_handle), "kc_set_stream")

    def reset(self, new_kmer_len=0):
        check(lib().kc_reset(self._h, new_kmer_len), "kc_reset")
        if self._tuning:
            self.set_tuning(**self._tuning)
        if new_kmer_len:
            self.k = new_kmer_len
            self.nl = lib().kc_num_longs(new_kmer_len)
            self.rec_nl = lib().kc_record_longs(new_kmer_len)

    def _torch_device(self):
        return "cuda:%d" % self.device

    def _out(self, dev, n, dtype, **kw):
        """an output array of the call's side (_Out): on this counter's device, or host memory"""
        return _Out(self._torch_device() if dev else None, n, dtype, **kw)

    def _hand_over(self, dev=True):
        """The hand-over from torch to the library in a call on the device side: the input and the fresh arrays are
        torch's until its current stream on this counter's device has nothing more to do with them."""
        if dev:
            import torch
            torch.cuda.current_stream(self.device).synchronize()

    def submit_reads(self, bases, quals, offsets, nreads=None):
        pb, pq, po, n, dev = _reads(bases, quals, offsets, nreads)
        check(lib().kc_submit_reads(self._h, pb, pq, po, n, 1 if dev else 0), "kc_submit_reads")

    def submit_packed_reads(self, packed, offsets, nreads=None):
        """PackedRead bytes (base | quality<<3, src/packed_reads.cpp:99-126) + offsets."""
        pp, _, po, n, dev = _reads(packed, None, offsets, nreads)
        check(lib().kc_submit_packed_reads(self._h, pp, po, n, 1 if dev else 0), "kc_submit_packed_reads")

    def merge_pairs(self, bases, quals, offsets, npairs=None, min_kmer_len=0):
        """Overlap merge of interleaved pairs on the device (kc_merge_pairs): returns (packed u8, offsets int64) as device
        tensors holding exactly the output, ready for submit_packed_reads, and the counters as a dict.  Host arrays are
        staged; min_kmer_len 0 = this counter's k."""
        pb, pq, po, nreads, dev = _reads(bases, quals, offsets, None if npairs is None else 2 * npairs)
        n = nreads // 2
        total = _span(offsets, 2 * n)
        packed, outo = self._out(True, total, np.uint8, pad=True), self._out(True, 2 * n + 1, np.uint64)
        nr, nb, st = C.c_uint64(0), C.c_uint64(0), kc_merge_stats()
        check(lib().kc_merge_pairs(self._h, pb, pq, po, n, 1 if dev else 0, min_kmer_len, packed.ptr, total, outo.ptr, 2 * n, C.byref(nr),
                                   C.byref(nb), C.byref(st)), "kc_merge_pairs")
        return packed.first(nb.value), outo.first(nr.value + 1), _stats_dict(st)

    def load_adapters(self, text_or_path, adapter_k=0, blastn_scores=False):
        """Load an adapter set into this counter (kc_adapters_load): FASTA text as bytes, or the path of a FASTA file as
        str.  adapter_k 0 = this counter's k; blastn_scores: align with 2/3/5/2/1 instead of 1/1/1/1/1.  The set stays
        over reset(); loading again replaces it.  Returns the loader's counts."""
        data = _adapter_text(text_or_path)
        return _adapter_counts("kc_adapters_load", self._h, data, len(data), adapter_k, _lib.KC_ADAPTERS_BLASTN_SCORES if blastn_scores else 0)

    def clear_adapters(self):
        check(lib().kc_adapters_clear(self._h), "kc_adapters_clear")

    def trim_adapters(self, bases, quals, offsets, paired=True, nreads=None):
        """Adapter trimming of interleaved reads on the device (kc_trim_adapters): Adapters::trim_pair over reads
        (2p, 2p+1), or with paired=False Adapters::trim per read.  Returns (bases u8, quals u8, offsets int64) as device
        tensors in the input's layout, ready for merge_pairs or submit_reads, and the counters as a dict.  Host arrays
        are staged."""
        pb, pq, po, n, dev = _reads(bases, quals, offsets, nreads)
        total = _span(offsets, n)
        ob, oq = self._out(True, total, np.uint8, pad=True), self._out(True, total, np.uint8, pad=True)
        oo = self._out(True, n + 1, np.uint64)
        nb, st = C.c_uint64(0), kc_trim_stats()
        self._hand_over()
        check(lib().kc_trim_adapters(self._h, pb, pq, po, n, 1 if dev else 0, _lib.KC_TRIM_PAIRED if paired else 0, ob.ptr, oq.ptr, total,
                                     oo.ptr, C.byref(nb), C.byref(st)), "kc_trim_adapters")
        return ob.first(nb.value), oq.first(nb.value), oo.a, _stats_dict(st)

    def fastq_to_packed(self, text, partial=False):
        """FASTQ text parsed on the device (kc_fastq_to_packed_device): returns (packed u8, offsets int64) as device
        tensors holding exactly kc_fastq_to_packed's output, ready for submit_packed_reads, and with partial=True also
        `consumed`, the byte past the last whole record (only whole records are parsed; the caller carries the tail).
        text: bytes, a numpy uint8 array (copied to the device) or a uint8 device tensor (read in place)."""
        pt, n, dev, keep = _text(text)
        packed, offs = self._out(True, n, np.uint8, pad=True), self._out(True, n // 4 + 2, np.uint64)
        nr, nb, cons = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._hand_over()
        check(lib().kc_fastq_to_packed_device(self._h, pt, n, 1 if dev else 0, _lib.KC_FASTQ_PARTIAL if partial else 0, packed.ptr, n,
                                              offs.ptr, n // 4 + 1, C.byref(nr), C.byref(nb), C.byref(cons)), "kc_fastq_to_packed_device")
        del keep
        out = (packed.first(nb.value), offs.first(nr.value + 1))
        return out + (cons.value,) if partial else out

    def fastq_pairs(self, text1, text2=None, partial=False):
        """Paired FASTQ text parsed on the device (kc_fastq_pairs_device; text2 None = text1 interleaved): returns
        (bases u8, quals u8, offsets int64) device tensors holding exactly kc_fastq_pairs' output, ready for merge_pairs,
        and with partial=True also (consumed1, consumed2), the bytes of each text taken (consumed2 None for one text)."""
        p1, n1, dev, keep1 = _text(text1)
        p2, n2, _, keep2 = _text(text2) if text2 is not None else (None, 0, dev, None)
        if text2 is not None and _text_on_device(text2) != dev:
            raise ValueError("text1 and text2 must both be host or both be device memory")
        if text2 is not None and not p2:  # an empty second file is still a second file: NULL text2 would mean interleaved
            keep2 = self._out(dev, 1, np.uint8, zeroed=True)
            p2 = keep2.ptr
        n = n1 + n2
        bases, quals = self._out(True, n, np.uint8, pad=True), self._out(True, n, np.uint8, pad=True)
        offs = self._out(True, n // 4 + 2, np.uint64)
        nr, nb, c1, c2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._hand_over()
        check(lib().kc_fastq_pairs_device(self._h, p1, n1, p2, n2, 1 if dev else 0, _lib.KC_FASTQ_PARTIAL if partial else 0, bases.ptr,
                                          quals.ptr, n, offs.ptr, n // 4 + 1, C.byref(nr), C.byref(nb), C.byref(c1), C.byref(c2)),
              "kc_fastq_pairs_device")
        del keep1, keep2
        out = (bases.first(nb.value), quals.first(nb.value), offs.first(nr.value + 1))
        return out + ((c1.value, None if text2 is None else c2.value),) if partial else out

    def submit_fastq(self, path_or_fileobj, block_bytes=1 << 30):
        """Stream a FASTQ file into the counter: block by block through fastq_to_packed(partial=True) and
        submit_packed_reads, the unfinished tail carried into the next block, the last call without the flag.
        Returns the number of reads submitted."""
        own = not hasattr(path_or_fileobj, "read")
        f = open(path_or_fileobj, "rb") if own else path_or_fileobj
        total, tail = 0, b""
        try:
            while True:
                chunk = f.read(block_bytes)
                buf = tail + chunk if tail else chunk
                if not chunk:  # end of file: the rest must be whole records
                    packed, offs = self.fastq_to_packed(buf)
                    tail = b""
                else:
                    packed, offs, consumed = self.fastq_to_packed(buf, partial=True)
                    tail = buf[consumed:]
                nr = offs.numel() - 1
                if nr:
                    self.submit_packed_reads(packed, offs, nreads=nr)
                    total += nr
                if not chunk:
                    return total
        finally:
            if own:
                f.close()

    def submit_seq_block(self, seqs, length=None):
        if isinstance(seqs, (bytes, bytearray)):
            buf = np.frombuffer(bytes(seqs), dtype=np.uint8)
            check(lib().kc_submit_seq_block(self._h, buf.ctypes.data, len(buf), 0), "kc_submit_seq_block")
            return
        p, dev = _ptr(seqs)
        n = len(seqs) if length is None else length
        check(lib().kc_submit_seq_block(self._h, p, n, 1 if dev else 0), "kc_submit_seq_block")

    def wire_unit(self):
        """(words, records, pieces) of kc_extract_partition / kc_insert_records: a unit of `words` words holds `records`
        records, every destination gets `pieces` pieces -- (kc_record_longs, 1, 1) for k-mer records, (3, 4, 2..16) where a
        context created with wire_units=True exchanges six-byte records (kc_wire_unit)."""
        w, r, q = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().kc_wire_unit(self._h, C.byref(w), C.byref(r), C.byref(q)), "kc_wire_unit")
        return w.value, r.value, q.value

    def partition_owner(self, kmer_words):
        """the shard kc_extract_partition sends this canonical k-mer to (kc_partition_owner)"""
        w = np.ascontiguousarray(kmer_words, dtype=np.uint64)
        o = C.c_int(-1)
        check(lib().kc_partition_owner(self._h, w.ctypes.data, C.byref(o)), "kc_partition_owner")
        return o.value

    def extract_partition(self, bases, quals, offsets, records, seg_capacity, nreads=None):
        """records: device buffer of rank_n*pieces*seg_capacity*unit_words u64 (wire_unit()).  Returns the units of every
        piece, destination after destination."""
        pb, pq, po, n, dev = _reads(bases, quals, offsets, nreads)
        pr, _ = _ptr(records)
        counts = np.zeros(self.rank_n * (self.wire_unit()[2] if self._wire_units else 1), dtype=np.uint64)
        check(lib().kc_extract_partition(self._h, pb, pq, po, n, 1 if dev else 0, pr, seg_capacity, counts.ctypes.data),
              "kc_extract_partition")
        return counts

    def build_supermers(self, block, capacity=None):
        """ParseAndPackGPUDriver::process_seq_block + pack_seq_block on a '_'-joined case-masked block (bytes):
        returns (targets i32, offsets i32, lens u16, num_valid_kmers, packed u8[(len+1)//2])."""
        blk = np.frombuffer(block, dtype=np.uint8) if isinstance(block, (bytes, bytearray)) else np.ascontiguousarray(block, dtype=np.uint8)
        cap = capacity if capacity is not None else max(16, len(blk))
        out = np.zeros(cap, dtype=np.dtype([("target", np.int32), ("offset", np.int32), ("len", np.uint16), ("pad", np.uint16)]))
        packed = np.zeros((len(blk) + 1) // 2, dtype=np.uint8)
        n, nk = C.c_uint32(0), C.c_uint32(0)
        check(lib().kc_build_supermers(self._h, blk.ctypes.data, len(blk), 0, out.ctypes.data, cap, C.byref(n), C.byref(nk),
                                       packed.ctypes.data), "kc_build_supermers")
        out = out[:n.value]
        return out["target"].copy(), out["offset"].copy(), out["len"].copy(), nk.value, packed

    def begin_ctg_kmers(self, max_ctg_kmers):
        """HashTableInserter::init_ctg_kmers: room for that many distinct contig k-mers (before finalize)."""
        check(lib().kc_begin_ctg_kmers(self._h, int(max_ctg_kmers)), "kc_begin_ctg_kmers")

    def submit_ctgs(self, ctgs, depths):
        """process_seq(ctg.seq, ctg.depth) for every contig: a '_'-joined block with its per-character depths."""
        block = b"_".join(c.encode() if isinstance(c, str) else c for c in ctgs) + b"_"
        dd = np.zeros(len(block), dtype=np.uint16)
        at = 0
        for c, d in zip(ctgs, depths):
            dd[at:at + len(c) + 1] = d
            at += len(c) + 1
        blk = np.frombuffer(block, dtype=np.uint8)
        check(lib().kc_submit_ctg_block(self._h, blk.ctypes.data, dd.ctypes.data, len(blk), 0), "kc_submit_ctg_block")

    def ctg_stats(self):
        """(distinct contig k-mers in the contig table, characters submitted)"""
        d, n = C.c_uint64(0), C.c_uint64(0)
        check(lib().kc_ctg_stats(self._h, C.byref(d), C.byref(n)), "kc_ctg_stats")
        return int(d.value), int(n.value)

    def submit_packed_supermers(self, packed):
        """4-bit packed supermers joined by the byte '_' (HashTableGPUDriver::insert_supermer's buffer)."""
        pp, dev = _ptr(packed)
        n = packed.numel() if hasattr(packed, "numel") else len(packed)
        check(lib().kc_submit_packed_supermers(self._h, pp, n, 1 if dev else 0), "kc_submit_packed_supermers")

    def insert_records(self, records, n):
        pr, _ = _ptr(records)
        check(lib().kc_insert_records(self._h, pr, n), "kc_insert_records")

    def insert_record_pieces(self, records, piece_stride_units, units):
        """kc_insert_record_pieces: pieces of `units[j]` units that lie piece_stride_units units apart, from `records` on"""
        pr, _ = _ptr(records)
        u = np.ascontiguousarray(units, dtype=np.uint64)
        check(lib().kc_insert_record_pieces(self._h, pr, int(piece_stride_units), len(u), u.ctypes.data), "kc_insert_record_pieces")

    # ---- the single-pass shard flow (ownership by level-1 bucket) ----
    def shard_extract(self, bases, quals, offsets, segments, seg_words, nreads=None):
        """segments: device buffer of rank_n*seg_words u64.  Returns the words to ship per destination."""
        pb, pq, po, n, dev = _reads(bases, quals, offsets, nreads)
        ps, _ = _ptr(segments)
        words = np.zeros(self.rank_n, dtype=np.uint64)
        check(lib().kc_shard_extract(self._h, pb, pq, po, n, 1 if dev else 0, ps, seg_words, words.ctypes.data), "kc_shard_extract")
        return words

    def shard_extract_seq_block(self, seqs, segments, seg_words):
        """The same from a '_'-joined case-masked block (bytes, or a device tensor of them)."""
        if isinstance(seqs, (bytes, bytearray)):
            buf = np.frombuffer(bytes(seqs), dtype=np.uint8)
            p, dev, n = buf.ctypes.data, False, len(buf)
        else:
            (p, dev), n = _ptr(seqs), len(seqs)
        ps, _ = _ptr(segments)
        words = np.zeros(self.rank_n, dtype=np.uint64)
        check(lib().kc_shard_extract_seq_block(self._h, p, n, 1 if dev else 0, ps, seg_words, words.ctypes.data), "kc_shard_extract_seq_block")
        return words

    def shard_reserve(self, nwords, device=None):
        """Context-owned device memory for nwords incoming u64, as an int64 torch tensor viewing it (no copy)."""
        import torch
        p = C.c_void_p(0)
        check(lib().kc_shard_reserve(self._h, int(nwords), C.byref(p)), "kc_shard_reserve")
        if not nwords:
            return torch.empty(0, dtype=torch.int64, device=device or self._torch_device())
        return _DeviceWords(p.value, int(nwords), device or self._torch_device()).tensor()

    def shard_commit(self, segment, nwords):
        ps, _ = _ptr(segment)
        check(lib().kc_shard_commit(self._h, ps, int(nwords)), "kc_shard_commit")

    def shard_capacity(self):
        """Distinct k-mers this shard's regions hold in the single-pass flow (kc_shard_capacity)."""
        v = C.c_uint64(0)
        check(lib().kc_shard_capacity(self._h, C.byref(v)), "kc_shard_capacity")
        return v.value

    def shard_owner(self, kmer_words):
        w = np.ascontiguousarray(kmer_words, dtype=np.uint64)
        o = C.c_int(-1)
        check(lib().kc_shard_owner(self._h, w.ctypes.data, C.byref(o)), "kc_shard_owner")
        return o.value

    def flush(self):
        check(lib().kc_flush(self._h), "kc_flush")

    def finalize(self):
        r = kc_result()
        check(lib().kc_finalize(self._h, C.byref(r)), "kc_finalize")
        self._res = r
        return r

    def results(self):
        """Host copies: keys (n, num_longs) u64, counts u16, left u8, right u8 (unordered)."""
        r = self.finalize()
        n = int(r.n)
        keys = np.empty((n, self.nl), dtype=np.uint64)
        counts = np.empty(n, dtype=np.uint16)
        left = np.empty(n, dtype=np.uint8)
        right = np.empty(n, dtype=np.uint8)
        check(lib().kc_copy_results(self._h, keys.ctypes.data, counts.ctypes.data, left.ctypes.data, right.ctypes.data),
              "kc_copy_results")
        return keys, counts, left, right

    def lookup(self, queries):
        """queries: (n, num_longs) uint64 k-mers in either orientation (host array).  Returns counts u16, left u8,
        right u8; count 0 = not among the results (KmerDHT::get_kmer_count, kmer_dht.cpp:228-245)."""
        self.finalize()
        qa = np.ascontiguousarray(queries, dtype=np.uint64).reshape(-1, self.nl)
        n = len(qa)
        counts = np.zeros(n, dtype=np.uint16)
        left = np.zeros(n, dtype=np.uint8)
        right = np.zeros(n, dtype=np.uint8)
        check(lib().kc_lookup(self._h, qa.ctypes.data, n, 0, counts.ctypes.data, left.ctypes.data, right.ctypes.data), "kc_lookup")
        return counts, left, right

    def sorted_results(self):
        keys, counts, left, right = self.results()
        order = np.lexsort([keys[:, j] for j in range(self.nl - 1, -1, -1)]) if len(counts) else np.zeros(0, dtype=np.int64)
        return keys[order], counts[order], left[order], right[order]

    def dump_table(self):
        n = C.c_uint64(0)
        check(lib().kc_dump_table(self._h, None, None, None, C.byref(n)), "kc_dump_table")
        keys = np.empty((n.value, self.nl), dtype=np.uint64)
        counts = np.empty(n.value, dtype=np.uint16)
        exts = np.empty((n.value, 8), dtype=np.uint16)
        if n.value:
            check(lib().kc_dump_table(self._h, keys.ctypes.data, counts.ctypes.data, exts.ctypes.data, C.byref(n)), "kc_dump_table")
        order = np.lexsort([keys[:, j] for j in range(self.nl - 1, -1, -1)]) if n.value else np.zeros(0, dtype=np.int64)
        return keys[order], counts[order], exts[order]

    def stats(self):
        s = kc_stats()
        check(lib().kc_get_stats(self._h, C.byref(s)), "kc_get_stats")
        return _stats_dict(s)

    def arena_probe_rate(self):
        """TB/s of level 1's write pattern on the level-1 arena this context chose (0.0: no probe ran)."""
        v = C.c_double(0.0)
        check(lib().kc_arena_probe_rate(self._h, C.byref(v)), "kc_arena_probe_rate")
        return float(v.value)

    def kernel_times(self, clear=False):
        """{kernel name: (launches, total_ms)} from HIP events on the launch stream (needs time_kernels=True)."""
        n = C.c_int(0)
        check(lib().kc_get_kernel_times(self._h, None, 0, C.byref(n)), "kc_get_kernel_times")  # how many entries it has
        arr = (kc_kernel_time * n.value)()
        check(lib().kc_get_kernel_times(self._h, arr, len(arr), C.byref(n)), "kc_get_kernel_times")
        out = {x.name.decode(): (int(x.launches), float(x.total_ms)) for x in arr}
        if clear:
            check(lib().kc_clear_kernel_times(self._h), "kc_clear_kernel_times")
        return out

    def synth_reads_device(self, d_bases, d_quals, d_offsets, nreads, first_read=0, params=None):
        p = params or synth_params()
        check(lib().kc_synth_reads_device(self._h, C.byref(p), first_read, nreads, _ptr(d_bases)[0], _ptr(d_quals)[0],
                                          _ptr(d_offsets)[0]), "kc_synth_reads_device")

    def dump_lines(self):
        """The reference's dump format, one "KMER count L R" per k-mer (kmer_dht.cpp:273-297), sorted."""
        keys, counts, left, right = self.sorted_results()
        return ["%s %d %s %s" % (kmer_to_string(keys[i], self.k), counts[i], chr(left[i]), chr(right[i]))
                for i in range(len(counts))]


    def sort_results(self):
        """Order the results by key on the device (kc_sort_results): the order sorted_results() computes on the host.
        Returns the refreshed kc_result; one obtained earlier is invalid."""
        self.finalize()
        r = kc_result()
        check(lib().kc_sort_results(self._h, C.byref(r)), "kc_sort_results")
        self._res = r
        return r

    def dump_text(self, first=0, count=None, sort=True):
        """The dump text of results [first, first + count) as bytes, formatted on the device (kc_dump_text_device): what
        "".join(line + "\n" for line in dump_lines()) gives for the whole.  sort=False: the results' current order."""
        r = self.sort_results() if sort else self.finalize()
        if count is None:
            count = int(r.n) - first
        nb = C.c_uint64(0)
        check(lib().kc_dump_text_device(self._h, first, count, None, 0, C.byref(nb)), "kc_dump_text_device")
        if not nb.value:
            return b""
        text = self._out(True, nb.value, np.uint8)
        self._hand_over()
        check(lib().kc_dump_text_device(self._h, first, count, text.ptr, nb.value, C.byref(nb)), "kc_dump_text_device")
        return text.a.cpu().numpy().tobytes()

    def _unitigs(self, with_depths, with_sums):
        self.finalize()
        L = lib()
        nu, nb, st = C.c_uint64(0), C.c_uint64(0), kc_unitig_stats()
        check(L.kc_build_unitigs(self._h, None, 0, None, None, 0, None, C.byref(nu), C.byref(nb), C.byref(st)), "kc_build_unitigs")
        seqs = self._out(True, nb.value, np.uint8)
        # zeroed: without unitigs seqs has no address, the call is one more size query and offsets[0] is not written
        offsets = self._out(True, nu.value + 1, np.uint64, zeroed=True)
        depths = self._out(True, nb.value, np.uint16) if with_depths else None
        sums = self._out(True, nu.value, np.uint64) if with_sums else None
        self._hand_over()
        check(L.kc_build_unitigs(self._h, seqs.ptr, nb.value, depths.ptr if with_depths else None, offsets.ptr, nu.value,
                                 sums.ptr if with_sums else None, C.byref(nu), C.byref(nb), C.byref(st)), "kc_build_unitigs")
        self._res = None  # the results may have moved (kc_sort_results)
        return seqs.a, depths.a if with_depths else None, offsets.a, sums.a if with_sums else None, _stats_dict(st)

    def unitigs(self):
        """The unitigs of the results, built on the device (kc_build_unitigs): (seqs, offsets,
        kmer_sums, stats) -- seqs a uint8 device tensor in the seq-block format (every unitig followed by '_'), offsets an
        int64 device tensor of len(unitigs) + 1 starts, kmer_sums an int64 device tensor of the summed counts, stats a
        dict of kc_unitig_stats.  A size query, then the call.  The results end up in key order (sort_results())."""
        seqs, _, offsets, sums, st = self._unitigs(False, True)
        return seqs, offsets, sums, st

    def unitig_block(self):
        """(seqs, depths): the unitigs as a device seq block and, per byte, the unitig's depth as int16 bits of the
        uint16 value (0 on a separator) -- what kc_submit_ctg_block takes with on_device = 1 (submit_ctg_block)."""
        seqs, depths, _, _, _ = self._unitigs(True, False)
        return seqs, depths

    def unitig_strings(self):
        """Host list of (sequence, kmer_sum), in the output's order: for tests and small inputs."""
        seqs, offsets, sums, _ = self.unitigs()
        return list(zip(_block_strings(seqs, offsets), sums.cpu().tolist()))

    def index_contigs(self, seqs, offsets):
        """Seed index over a block of contigs (kc_ctg_index_build): seqs a uint8 seq block (every
        contig followed by '_'), offsets its len(contigs) + 1 starts as 64-bit integers -- numpy arrays, or device tensors
        as unitigs() returns them.  The counter keeps its own copy; an earlier index is replaced.  Returns
        kc_ctg_index_stats as a dict."""
        ps, dev_s = _ptr(seqs)
        po, dev_o = _ptr(offsets)
        dev = _side("seqs", dev_s, offsets=(dev_o, True))
        n = len(offsets) - 1
        nbytes = seqs.numel() if dev else len(seqs)
        st = kc_ctg_index_stats()
        self._hand_over(dev)
        check(lib().kc_ctg_index_build(self._h, ps if nbytes else None, nbytes, po, n, 1 if dev else 0, C.byref(st)), "kc_ctg_index_build")
        return _stats_dict(st)

    def index_unitigs(self):
        """unitigs() straight into the seed index, on the device.  Returns kc_ctg_index_stats as a dict."""
        seqs, _, offsets, _, _ = self._unitigs(False, False)
        return self.index_contigs(seqs, offsets)

    def clear_contig_index(self):
        check(lib().kc_ctg_index_clear(self._h), "kc_ctg_index_clear")

    def align_reads(self, bases, offsets, seed_space=1, max_mismatches=None, nreads=None):
        """Reads onto the indexed contigs (kc_align_reads): a size query, then the call.  bases
        uint8 ASCII, offsets nreads + 1 64-bit integers.  Returns (alns, read_first, stats): for host arrays alns is a
        numpy structured array (ALN_DTYPE) and read_first a uint64 array; for device tensors alns is a uint8 device tensor
        of 32-byte records and read_first an int64 device tensor.  max_mismatches None keeps every candidate."""
        pb, _, po, n, dev_b = _reads(bases, None, offsets, nreads)
        dev = _side("offsets", _ptr(offsets)[1], bases=(dev_b, n))
        mm = _lib.KC_ALIGN_KEEP_ALL if max_mismatches is None else max_mismatches
        head = (self._h, pb, po, n, 1 if dev else 0, seed_space, mm)
        na, st = C.c_uint64(0), kc_align_stats()
        self._hand_over(dev)
        check(lib().kc_align_reads(*head, None, 0, None, C.byref(na), C.byref(st)), "kc_align_reads")
        alns, first = self._out(dev, na.value, ALN_DTYPE, pad=True), self._out(dev, n + 1, np.uint64)
        self._hand_over(dev)  # fresh arrays
        check(lib().kc_align_reads(*head, alns.ptr, na.value, first.ptr, C.byref(na), C.byref(st)), "kc_align_reads")
        return alns.first(na.value), first.a, _stats_dict(st)

    def align_gapped(self, bases, offsets, alns, pad=16, scores=None, always_dp=False):
        """Gapped refinement of align_reads' records (kc_align_gapped): the same reads and the
        records as align_reads returned them -- host arrays (alns a structured array of ALN_DTYPE) or device tensors (alns
        a uint8 tensor of 32-byte records).  scores: (match, mismatch, gap open, gap extend, ambiguity), by default
        BLASTN_ALN_SCORES.  Returns (gap_alns, stats): one record per input record, in the same order -- a structured
        array of GAP_ALN_DTYPE for host arrays, a uint8 device tensor of 32-byte records for device tensors."""
        pb, _, po, n, dev_b = _reads(bases, None, offsets)
        pa, n_alns, dev_a = _records("alns", alns, ALN_DTYPE)
        dev = _side("offsets", _ptr(offsets)[1], alns=(dev_a, n_alns), bases=(dev_b, n and len(bases)))
        sc = kc_aln_scores(*(BLASTN_ALN_SCORES if scores is None else scores))
        st = kc_gap_stats()
        out = self._out(dev, n_alns, GAP_ALN_DTYPE, pad=True)
        self._hand_over(dev)
        check(lib().kc_align_gapped(self._h, pb, po, n, pa, n_alns, 1 if dev else 0, pad, C.byref(sc),
                                    _lib.KC_GAP_ALWAYS_DP if always_dp else 0, out.ptr, C.byref(st)), "kc_align_gapped")
        return out.first(), _stats_dict(st)

    def contig_index_info(self):
        """(nbytes, n_ctgs) of the kept contig index (kc_ctg_index_info): the sizes of aln_depths' arrays."""
        nb, nc = C.c_uint64(0), C.c_uint64(0)
        check(lib().kc_ctg_index_info(self._h, C.byref(nb), C.byref(nc)), "kc_ctg_index_info")
        return int(nb.value), int(nc.value)

    def aln_depths(self, gap_alns, min_score=0, min_len=0, edge_clip=0, best_only=False, per_contig=False, nreads=None):
        """Per-base and per-contig depths from align_gapped's records (kc_aln_depths).  Returns
        (depths, ctgs, stats): depths one 16-bit value per byte of the indexed block -- what submit_ctg_block takes;
        with per_contig every byte holds its contig's mean -- and ctgs one CTG_DEPTH_DTYPE record per contig.  Host
        records give numpy arrays; a uint8 device tensor of records gives device tensors (depths int16 holding the
        16 bits, ctgs uint8 of 32-byte records).  best_only: only every read's best record counts (nreads: the reads
        the records index)."""
        pa, n, dev = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        if best_only and nreads is None:
            raise ValueError("best_only needs nreads")
        nbytes, n_ctgs = self.contig_index_info()
        flags = (_lib.KC_DEPTH_BEST_ONLY if best_only else 0) | (_lib.KC_DEPTH_PER_CONTIG if per_contig else 0)
        st = kc_depth_stats()
        depths, ctgs = self._out(dev, nbytes, np.uint16, pad=True), self._out(dev, n_ctgs, CTG_DEPTH_DTYPE, pad=True)
        self._hand_over(dev)
        check(lib().kc_aln_depths(self._h, pa, n, nreads or 0, 1 if dev else 0, min_score, min_len, edge_clip, flags, depths.ptr, ctgs.ptr,
                                  C.byref(st)), "kc_aln_depths")
        return depths.first(), ctgs.first(), _stats_dict(st)

    def pair_inserts(self, offsets, gap_alns, max_insert=_lib.KC_INSERT_MAX, min_score=0, min_len=0):
        """Every read's best record, every pair's class and the insert-size histogram (kc_pair_inserts; DESIGN.md
        section 17); reads 2p and 2p + 1 are mates.  Returns (hist, pairs, stats): hist max_insert + 1 counts, pairs one
        PAIR_DTYPE record per pair (host) or a uint8 device tensor of 16-byte records, hist an int64 device tensor then.
        stats: kc_insert_stats as a dict, cls a list by KC_PAIR_*, with mean and stddev of the proper pairs' inserts
        (0.0 without any) beside the integers."""
        pa, n, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        po, dev_o = _ptr(offsets)
        dev = _side("offsets", dev_o, gap_alns=(dev_a, n))
        nreads = len(offsets) - 1
        st = kc_insert_stats()
        hist, pairs = self._out(dev, max_insert + 1, np.uint64), self._out(dev, nreads // 2, PAIR_DTYPE, pad=True)
        self._hand_over(dev)
        check(lib().kc_pair_inserts(self._h, po, nreads, pa, n, 1 if dev else 0, min_score, min_len, max_insert, hist.ptr, pairs.ptr,
                                    C.byref(st)), "kc_pair_inserts")
        out = _stats_dict(st)
        proper = out["cls"][_lib.KC_PAIR_PROPER]
        out["mean"] = out["insert_sum"] / proper if proper else 0.0
        # the variance from exact integers: n * sum(x^2) - sum(x)^2 >= 0
        out["stddev"] = (proper * out["insert_sq_sum"] - out["insert_sum"] ** 2) ** 0.5 / proper if proper else 0.0
        return hist.a, pairs.first(), out

    def local_assm(self, bases, quals, offsets, gap_alns, pairs, ctg_depths=None, min_mer_len=13, max_mer_len=121, shift=8, max_walk_len=400,
                   max_insert=1000, min_qual=10, hi_qual=20, min_viable=2, viable_permille=200, max_cands=2000, table_budget_mb=0):
        """The indexed contigs, every end extended by a walk through the mers of the reads that hang over it and of the
        mates that fall beyond it (kc_local_assm).  bases / quals / offsets: the reads align_gapped
        took (quals None: every base is high quality); gap_alns its records, pairs pair_inserts' records, ctg_depths
        aln_depths' per-contig records (None: depth 0).  Returns (seqs, offsets, ends, stats): the new seq block and its
        len(contigs) + 1 starts -- what index_contigs and submit_ctg_block take -- one LASSM_END_DTYPE record per end
        (2u: left end of contig u, 2u + 1: right) and kc_lassm_stats as a dict, status a list by KC_LASSM_*.  Host arrays in
        give numpy arrays out; device tensors in give device tensors out (ends a uint8 tensor of 16-byte records, offsets
        int64).  The block is allocated at the indexed block's size plus a quarter; if that is too small the call is
        made once more with the size it reported."""
        pa, n_alns, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        pb, pq, po, nreads, dev_b = _reads(bases, quals, offsets)
        pp, npairs, dev_p = _records("pairs", pairs, PAIR_DTYPE)
        # the one record array whose contiguity has never been looked at, and whose address goes to the library as it is
        _, n_depths, dev_c = (None, 0, False) if ctg_depths is None else _records("ctg_depths", ctg_depths, CTG_DEPTH_DTYPE, contiguous=False)
        pc = _ptr(ctg_depths)[0]
        nbytes, n_ctgs = self.contig_index_info()
        n_bases = nreads and len(bases)
        dev = _side("offsets", _ptr(offsets)[1], gap_alns=(dev_a, n_alns), bases=(dev_b, n_bases),
                    quals=(_ptr(quals)[1], n_bases and quals is not None), pairs=(dev_p, npairs),
                    ctg_depths=(dev_c, n_ctgs and ctg_depths is not None))
        if npairs != nreads // 2:
            raise ValueError("pairs: a contiguous array of nreads / 2 16-byte records (PAIR_DTYPE)")
        if ctg_depths is not None and n_depths != n_ctgs:
            raise ValueError("ctg_depths: one 32-byte record (CTG_DEPTH_DTYPE) per indexed contig")
        prm = kc_lassm_params(min_mer_len, max_mer_len, shift, max_walk_len, max_insert, min_qual, hi_qual, min_viable, viable_permille,
                              max_cands, table_budget_mb, 0)
        st, nb = kc_lassm_stats(), C.c_uint64(0)
        offs_out, ends = self._out(dev, n_ctgs + 1, np.uint64), self._out(dev, 2 * n_ctgs, LASSM_END_DTYPE, pad=True)

        def call(capacity):
            seqs = self._out(dev, capacity, np.uint8, pad=True)
            self._hand_over(dev)
            rc = lib().kc_local_assm(self._h, pb, pq, po, nreads, pa, n_alns, pp, pc, 1 if dev else 0, C.byref(prm), seqs.ptr, capacity,
                                     offs_out.ptr, ends.ptr, C.byref(nb), C.byref(st))
            return rc, int(nb.value), seqs

        rc, told, seqs = _retry_on_capacity(nbytes + nbytes // 4, call, below=1 << 31)
        check(rc, "kc_local_assm")
        return seqs.first(told), offs_out.a, ends.first(), _stats_dict(st)

    def ctg_links(self, offsets, gap_alns, pairs=None, insert_avg=300, max_insert=1000, min_score=0, min_len=0, end_slack=5, max_overlap=200,
                  max_splint_gap=100, max_read_alns=8):
        """The links between the ends of the indexed contigs (kc_ctg_links): splints from reads
        aligned across two contigs, spans from pairs whose mates' best records lie on different contigs.  offsets: the
        reads' (2p and 2p + 1 are mates); gap_alns align_gapped's records in any order; pairs pair_inserts' records
        (None: no spans); insert_avg the insert size a span's gap is measured against.  Returns (links, end_first, stats,
        gap): every link once in each direction, ordered by (from, to) -- LINK_DTYPE records for host arrays, a uint8
        device tensor of 48-byte records for device tensors -- end_first the index of every end's first record and the
        total (uint64 array / int64 tensor; end 2u is the left end of contig u, 2u + 1 its right end), kc_link_stats as a
        dict, and gap a float64 numpy column: a link's mean splint gap where it has splints, else its mean span gap.  The
        records are allocated at four a contig; if that is too few the call is made once more with the number it reported."""
        pa, n_alns, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        po, dev_o = _ptr(offsets)
        nreads = len(offsets) - 1
        pp, npairs, dev_p = (None, 0, False) if pairs is None else _records("pairs", pairs, PAIR_DTYPE)
        dev = _side("offsets", dev_o, gap_alns=(dev_a, n_alns), pairs=(dev_p, npairs))
        if pairs is not None and npairs != nreads // 2:
            raise ValueError("pairs: a contiguous array of nreads / 2 16-byte records (PAIR_DTYPE)")
        _, n_ctgs = self.contig_index_info()
        prm = kc_link_params(min_score, min_len, end_slack, max_overlap, max_splint_gap, insert_avg, max_insert, max_read_alns, 0)
        st, n = kc_link_stats(), C.c_uint64(0)
        end_first = self._out(dev, 2 * n_ctgs + 1, np.uint64)

        def call(capacity):
            links = self._out(dev, capacity, LINK_DTYPE, pad=True)
            self._hand_over(dev)
            rc = lib().kc_ctg_links(self._h, po, nreads, pa, n_alns, pp, 1 if dev else 0, C.byref(prm), links.ptr, capacity, end_first.ptr,
                                    C.byref(n), C.byref(st))
            return rc, int(n.value), links

        rc, n_links, links = _retry_on_capacity(4 * n_ctgs + 16, call)  # two records an end: a chain of contigs and as much again
        check(rc, "kc_ctg_links")
        links = links.first(n_links)
        host = links.cpu().numpy().view(LINK_DTYPE) if dev else links
        gap = np.zeros(n_links, dtype=np.float64)
        if n_links:
            s, m = host["splints"].astype(np.float64), host["spans"].astype(np.float64)
            gap = np.where(s > 0, host["splint_gap_sum"] / np.maximum(s, 1), host["span_gap_sum"] / np.maximum(m, 1))
        return links, end_first.a, _stats_dict(st), gap

    def scaffolds(self, links, min_splints=1, min_spans=2, max_second_permille=0, overlap_slack=0):
        """The scaffolds the links give over the indexed contigs (kc_scaffold): one partner per contig
        end (a link qualifies with min_splints splints or min_spans spans; an end whose second-best link has more than
        max_second_permille thousandths of the best's support is left alone), claimed overlaps checked against the text
        up to overlap_slack bases either way, the chosen edges walked into paths.  links: ctg_links' records (LINK_DTYPE
        array, or the uint8 device tensor).  Returns (seqs, offsets, scaffolds, members, stats): the seq block index_contigs
        takes as it is, SCAFFOLD_DTYPE and MEMBER_DTYPE records -- numpy for host input; uint8 / int64 device tensors and
        uint8 tensors of 32- and 16-byte records for a device tensor -- and kc_scaf_stats as a dict.  A size query first,
        then the call."""
        pl, n_links, dev = _records("links", links, LINK_DTYPE)
        _, n_ctgs = self.contig_index_info()
        prm = _lib.kc_scaf_params(min_splints, min_spans, max_second_permille, overlap_slack, 0)
        st, ns, nb = _lib.kc_scaf_stats(), C.c_uint64(0), C.c_uint64(0)
        head, tail = (self._h, pl, n_links, 1 if dev else 0, C.byref(prm)), (None, C.byref(ns), C.byref(nb), C.byref(st))
        self._hand_over(dev)
        check(lib().kc_scaffold(*head, None, 0, None, None, None, *tail), "kc_scaffold")
        n_scaf, nbytes = int(ns.value), int(nb.value)
        seqs, offsets = self._out(dev, nbytes, np.uint8), self._out(dev, n_scaf + 1, np.uint64)
        scafs, members = self._out(dev, n_scaf, SCAFFOLD_DTYPE, pad=True), self._out(dev, n_ctgs, MEMBER_DTYPE, pad=True)
        self._hand_over(dev)  # fresh arrays
        check(lib().kc_scaffold(*head, seqs.ptr, nbytes, offsets.ptr, scafs.ptr, members.ptr, *tail), "kc_scaffold")
        return seqs.a, offsets.a, scafs.first(), members.first(), _stats_dict(st)

    def scaffold_strings(self, links, **kw):
        """The scaffolds' texts as Python strings (for tests and small inputs): scaffolds() without its records."""
        return _block_strings(*self.scaffolds(links, **kw)[:2])

    def close_gaps(self, bases, offsets, gap_alns, scaffolds, members, min_reads=2, min_agree_permille=500, min_score=0, min_len=0, end_slack=5,
                   max_overlap=200, max_splint_gap=100, max_read_alns=8):
        """The scaffolds with their gaps closed from splint reads (kc_close_gaps): where at least
        min_reads reads aligned across a join's two contigs -- and min_agree_permille thousandths of the join's candidates --
        agree on the distance, the N run becomes the consensus of their bases, goes (the contigs abut) or becomes an overlap
        the text confirms.  bases / offsets: the reads; gap_alns: align_gapped's records; scaffolds / members: scaffolds()'
        records over the indexed contigs; the filter parameters are ctg_links'.  Returns (seqs, offsets, scaffolds, members,
        closures, stats): the seq block index_contigs takes as it is, SCAFFOLD_DTYPE, MEMBER_DTYPE and CLOSURE_DTYPE records
        -- numpy for host input; uint8 / int64 device tensors and uint8 tensors of 32-, 16- and 32-byte records for device
        tensors -- and kc_close_stats as a dict.  A size query first, then the call."""
        pa, n_alns, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        pb, _, po, nreads, dev_b = _reads(bases, None, offsets)
        # the library takes the scaffolds and the members as they are: they, and the offsets, count even where they are empty
        ps, n_scaf, dev_s = _records("scaffolds", scaffolds, SCAFFOLD_DTYPE, required=True)
        pm, n_members, dev_m = _records("members", members, MEMBER_DTYPE, required=True)
        dev = _side("bases", dev_b, offsets=(_ptr(offsets)[1], True), gap_alns=(dev_a, n_alns), scaffolds=(dev_s, True), members=(dev_m, True))
        _, n_ctgs = self.contig_index_info()
        if n_members != n_ctgs:
            raise ValueError("members: one record for each of the %d indexed contigs" % n_ctgs)
        prm = _lib.kc_close_params(min_score, min_len, end_slack, max_overlap, max_splint_gap, min_reads, min_agree_permille, max_read_alns, 0)
        st, nb = _lib.kc_close_stats(), C.c_uint64(0)
        head, tail = (self._h, pb, po, nreads, pa, n_alns, ps, n_scaf, pm, 1 if dev else 0, C.byref(prm)), (C.byref(nb), C.byref(st))
        self._hand_over(dev)
        check(lib().kc_close_gaps(*head, None, 0, None, None, None, None, *tail), "kc_close_gaps")
        nbytes = int(nb.value)
        seqs, offs_out = self._out(dev, nbytes, np.uint8), self._out(dev, n_scaf + 1, np.uint64)
        scafs, mem = self._out(dev, n_scaf, SCAFFOLD_DTYPE, pad=True), self._out(dev, n_ctgs, MEMBER_DTYPE, pad=True)
        clo = self._out(dev, n_ctgs, CLOSURE_DTYPE, pad=True)
        self._hand_over(dev)  # fresh arrays
        check(lib().kc_close_gaps(*head, seqs.ptr, nbytes, offs_out.ptr, scafs.ptr, mem.ptr, clo.ptr, *tail), "kc_close_gaps")
        return seqs.a, offs_out.a, scafs.first(), mem.first(), clo.first(), _stats_dict(st)

    def close_gaps_strings(self, bases, offsets, gap_alns, scaffolds, members, **kw):
        """The closed scaffolds' texts as Python strings (for tests and small inputs): close_gaps() without its records."""
        return _block_strings(*self.close_gaps(bases, offsets, gap_alns, scaffolds, members, **kw)[:2])

    def shuffle_reads(self, bases, quals, offsets, gap_alns, pairs, parts=1, remap=True):
        """The read pairs regrouped by their home contig (kc_shuffle_reads): a pair's home is the
        contig of the better of its mates' best records; homed pairs are ordered by (home, position on it), homeless
        ones keep their order, and both are dealt evenly over `parts` consecutive parts.  bases / quals / offsets: the
        reads (2p and 2p + 1 are mates; quals None: none come back); gap_alns align_gapped's records, pairs pair_inserts'.
        Returns a dict: bases, quals, offsets -- the reads in new order -- order (new pair -> old pair), home (new pair ->
        contig, KC_SHUFFLE_NO_HOME for none), part_starts (parts + 1 pair indices), gap_alns (the records with their read
        renumbered) and pairs (in new order), both None without remap, and stats (kc_shuffle_stats as a dict).  Host arrays
        in give numpy arrays out (GAP_ALN_DTYPE, PAIR_DTYPE records, uint32 order and home, uint64 offsets); device
        tensors in give device tensors out (uint8 tensors of records, int32 order and home holding the 32 bits, int64
        offsets and part_starts)."""
        pa, n_alns, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        pb, pq, po, nreads, dev_b = _reads(bases, quals, offsets)
        pp, npairs, dev_p = _records("pairs", pairs, PAIR_DTYPE)
        nbytes = len(bases)
        dev = _side("offsets", _ptr(offsets)[1], gap_alns=(dev_a, n_alns), bases=(dev_b, nbytes),
                    quals=(_ptr(quals)[1], nbytes and quals is not None), pairs=(dev_p, npairs))
        if npairs != nreads // 2:
            raise ValueError("pairs: a contiguous array of nreads / 2 16-byte records (PAIR_DTYPE)")
        if quals is not None and len(quals) != nbytes:
            raise ValueError("quals: as many bytes as bases")
        st = _lib.kc_shuffle_stats()
        # every output that may be empty is padded; the arrays that were not asked for stay None, here and in the result
        out = {"bases": self._out(dev, nbytes, np.uint8, pad=True),
               "quals": None if quals is None else self._out(dev, nbytes, np.uint8, pad=True),
               "offsets": self._out(dev, nreads + 1, np.uint64),
               "order": self._out(dev, npairs, np.uint32, pad=True),
               "home": self._out(dev, npairs, np.uint32, pad=True),
               "part_starts": self._out(dev, parts + 1, np.uint64),
               "gap_alns": self._out(dev, n_alns, GAP_ALN_DTYPE, pad=True) if remap else None,
               "pairs": self._out(dev, npairs, PAIR_DTYPE, pad=True) if remap else None}
        self._hand_over(dev)
        p = {k: v and v.ptr for k, v in out.items()}
        if not nbytes:  # no bases at all: the library takes no byte arrays then, in or out
            pb = pq = p["quals"] = None
        check(lib().kc_shuffle_reads(self._h, pb, pq, po, nreads, pa, n_alns, pp, 1 if dev else 0, parts, p["bases"], p["quals"], p["offsets"],
                                     p["order"], p["home"], p["part_starts"], p["gap_alns"], p["pairs"], C.byref(st)), "kc_shuffle_reads")
        out = {k: v and v.first() for k, v in out.items()}
        out["stats"] = _stats_dict(st)
        return out

    def _block(self, seqs, offsets, **others):
        """A seq block argument -> (address of seqs or None, bytes, address of offsets, contigs, on the device)."""
        ps, dev_s = _ptr(seqs)
        po, dev_o = _ptr(offsets)
        dev = _side("seqs", dev_s, offsets=(dev_o, True), **others)
        nbytes = seqs.numel() if dev else len(seqs)
        return (ps if nbytes else None), nbytes, po, len(offsets) - 1, dev

    def select_contigs(self, seqs, offsets, min_len=0, by_length=False):
        """Which contigs of a seq block are printed, in which order, and the assembly's statistics (kc_ctg_select; DESIGN.md
        section 23): a contig is selected iff it has at least min_len bases; order holds the selected contigs' block
        indices, in block order or, with by_length, longest first and equal lengths by index.  seqs / offsets: numpy
        arrays or device tensors, as index_contigs takes them.  Returns (order, stats): order a uint32 numpy array, or an
        int32 device tensor holding the 32 bits, and kc_asm_stats as a dict (N50, L50, the length classes, the Ns)."""
        ps, nbytes, po, n, dev = self._block(seqs, offsets)
        prm = _lib.kc_asm_params(min_len, _lib.KC_ASM_BY_LENGTH if by_length else 0)
        order = self._out(dev, n, np.uint32, pad=True)
        st, nsel = _lib.kc_asm_stats(), C.c_uint64(0)
        self._hand_over(dev)
        check(lib().kc_ctg_select(self._h, ps, nbytes, po, n, 1 if dev else 0, C.byref(prm), order.ptr, C.byref(nsel), C.byref(st)), "kc_ctg_select")
        return order.first(int(nsel.value)), _stats_dict(st)

    def dedup_contigs(self, seqs, offsets, depths=None, max_mismatches=0, duplicates_only=False, max_candidates=0):
        """A seq block without its duplicate and contained contigs (kc_ctg_dedup): a contig is removed
        iff its text or its reverse complement lies, with at most max_mismatches differing bytes, inside a contig that is
        longer, or as long and of smaller index (duplicates_only: as long).  seqs / offsets: numpy arrays or device tensors,
        as index_contigs takes them; depths: one uint16 per byte of the block, or None; max_candidates: the call's limit (0:
        2^26), KC_ERR_CAPACITY beyond it.  Returns (seqs, offsets, depths or None, records, stats): the block index_contigs,
        submit_ctg_block, select_contigs and fasta_text take as it is, one DEDUP_DTYPE record per input contig and
        kc_dedup_stats as a dict.  Host arrays in give numpy arrays out; device tensors in give device tensors out (offsets
        int64, depths int16, records a uint8 tensor of 32-byte records).  The block is allocated at the input's size, which
        the output never exceeds."""
        nd = 0 if depths is None else (depths.numel() if _ptr(depths)[1] else len(depths))
        ps, nbytes, po, n, dev = self._block(seqs, offsets, depths=(_ptr(depths)[1], nd))
        if depths is not None and nd != nbytes:
            raise ValueError("depths: one uint16 per byte of the block")
        prm = _lib.kc_dedup_params(max_mismatches, _lib.KC_DEDUP_DUPLICATES_ONLY if duplicates_only else 0, max_candidates)
        st, nk, nb = _lib.kc_dedup_stats(), C.c_uint64(0), C.c_uint64(0)
        recs, offs_out = self._out(dev, n, DEDUP_DTYPE, pad=True), self._out(dev, n + 1, np.uint64)

        def call(capacity):
            out = self._out(dev, capacity, np.uint8, pad=True), (None if depths is None else self._out(dev, capacity, np.uint16, pad=True))
            self._hand_over(dev)
            rc = lib().kc_ctg_dedup(self._h, ps, nbytes, po, n, _ptr(depths)[0], 1 if dev else 0, C.byref(prm), recs.ptr, out[0].ptr, capacity,
                                    offs_out.ptr, out[1] and out[1].ptr, C.byref(nk), C.byref(nb), C.byref(st))
            return rc, int(nb.value), out

        rc, told, (seqs_out, depths_out) = _retry_on_capacity(nbytes, call, below=1 << 31)
        check(rc, "kc_ctg_dedup")
        return seqs_out.first(told), offs_out.first(int(nk.value) + 1), depths_out and depths_out.first(told), recs.first(), _stats_dict(st)

    def dedup_strings(self, seqs, offsets, **kw):
        """The kept contigs' texts as Python strings (for tests and small inputs): dedup_contigs() without its records."""
        return _block_strings(*self.dedup_contigs(seqs, offsets, **kw)[:2])

    def kmer_depths(self, seqs, offsets, min_count=0, fill_mean=False, with_track=True, with_records=True):
        """The k-mer depth of sequences in the finished results (kc_seq_kmer_depths).  seqs / offsets:
        the bases and offsets of reads, or a seq block with its own offsets, numpy arrays or device tensors.  Returns
        (track, records, stats): track[p] the count of the window that starts at byte p, 0 where none does (fill_mean: the
        sequence's mean on every base byte, what submit_ctg_block takes), one KDEPTH_DTYPE record per sequence, and
        kc_kdepth_stats as a dict; a window counts as solid at min_count or more.  with_track / with_records False: None in
        that place, and the library is not asked for it.  Host arrays in give numpy arrays out; device tensors in give device
        tensors out (the track int16, records a uint8 tensor of 32-byte records)."""
        ps, nbytes, po, n, dev = self._block(seqs, offsets)
        prm = _lib.kc_kdepth_params(min_count, _lib.KC_KDEPTH_FILL_MEAN if fill_mean else 0)
        st = _lib.kc_kdepth_stats()
        track = self._out(dev, nbytes, np.uint16, pad=True) if with_track else None
        recs = self._out(dev, n, KDEPTH_DTYPE, pad=True) if with_records else None
        self._hand_over(dev)
        check(lib().kc_seq_kmer_depths(self._h, ps, nbytes, po, n, 1 if dev else 0, C.byref(prm), track and track.ptr, recs and recs.ptr,
                                       C.byref(st)), "kc_seq_kmer_depths")
        return track and track.first(), recs and recs.first(), _stats_dict(st)

    def correct_reads(self, bases, offsets, quals=None, min_count=2, min_gain=8, min_windows=2, rounds=3, max_qual=0, with_records=True,
                      with_fixes=False):
        """Reads with their substitution errors corrected from the finished results (kc_correct_reads).
        bases / offsets (and quals, only read with max_qual > 0): numpy arrays or device tensors, as kmer_depths takes them.  A
        window is solid at max(min_count, 1) or more; a weak run beside a solid window gives a site, the byte the first weak
        window holds and the anchor does not; a site is corrected to the one base that makes at least min(n, min_gain) leading
        windows of its range solid and more than either other base.  Returns (out, records, fixes, stats): out the corrected
        bases, of the same length and offsets; one CORRECT_REC_DTYPE record per sequence (with_records False: None); the
        CORRECT_FIX_DTYPE entries ordered by (round, seq, pos) (with_fixes False: None; True: room is found; a number: room for
        that many, KC_ERR_CAPACITY beyond); kc_correct_stats as a dict.  Host arrays in give numpy arrays out, device tensors
        in give device tensors out (records and fixes as uint8 tensors of 16-byte entries)."""
        ps, nbytes, po, n, dev = self._block(bases, offsets)
        pq, dev_q = _ptr(quals)
        if quals is not None and bool(dev_q) != bool(dev):
            raise ValueError("quals: a call's arrays are all host arrays or all device tensors")
        prm = _lib.kc_correct_params(min_count, min_gain, min_windows, rounds, max_qual, 0)
        out = self._out(dev, nbytes, np.uint8, pad=True)
        recs = self._out(dev, n, CORRECT_REC_DTYPE, pad=True) if with_records else None
        self._hand_over(dev)

        def call(capacity):
            st = _lib.kc_correct_stats()
            fixes = self._out(dev, capacity, CORRECT_FIX_DTYPE, pad=True) if with_fixes is not False else None
            self._hand_over(dev and fixes is not None)
            rc = lib().kc_correct_reads(self._h, ps, pq, nbytes, po, n, 1 if dev else 0, C.byref(prm), out.ptr, recs and recs.ptr,
                                        fixes and fixes.ptr, capacity, C.byref(st))
            return rc, fixes, st

        exact = with_fixes is not True and with_fixes is not False
        rc, fixes, st = call(int(with_fixes) if exact else nbytes // 16 + 1024)
        if rc == _lib.KC_ERR_CAPACITY and with_fixes is True:
            rc, fixes, st = call(nbytes * max(rounds, 1))  # a round changes a byte at most once
        check(rc, "kc_correct_reads")
        return out.first(), recs and recs.first(), fixes and fixes.first(int(st.accepted)), _stats_dict(st)

    def polish_contigs(self, bases, offsets, gap_alns, quals=None, min_score=0, min_len=0, edge_clip=0, max_mismatches=8, min_depth=3,
                       min_permille=700, min_qual=0, best_only=False, with_counts=False, with_records=True, with_fixes=True):
        """The indexed contigs polished from the pileup of align_gapped's records (kc_ctg_polish).  bases /
        offsets (and quals, only read with min_qual > 0): the reads the records index, numpy arrays or device tensors.  A record
        that passes the filter (min_score, min_len; best_only: and is its read's best), lies on one diagonal and differs from
        the contig in at most max_mismatches columns votes with its bases, edge_clip columns short of an end that is not the
        contig's; a column with min_depth votes or more whose winner has more votes than any other base and at least
        min_permille thousandths of them becomes the winner.  Substitutions only: the block keeps its length and offsets.
        Returns (block, counts, records, fixes, stats): the polished block; with_counts the four counts of every byte as a
        (nbytes, 4) uint16 array, saturated (else None); one POLISH_CTG_DTYPE record per contig (with_records False: None); the
        POLISH_FIX_DTYPE entries in ascending position (with_fixes False: None; True: room for every column; a number: room for
        that many, KC_ERR_CAPACITY beyond); kc_polish_stats as a dict.  Host arrays in give numpy arrays out, device tensors in
        give device tensors out (records and fixes as uint8 tensors, counts an int16 tensor of nbytes * 4 holding the bits)."""
        pa, n_alns, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        pb, pq, po, nreads, dev_b = _reads(bases, quals, offsets)
        nb_reads = len(bases)
        dev = _side("offsets", _ptr(offsets)[1], gap_alns=(dev_a, n_alns), bases=(dev_b, nb_reads), quals=(_ptr(quals)[1], nb_reads and quals is not None))
        if quals is not None and len(quals) != nb_reads:
            raise ValueError("quals: as many bytes as bases")
        nbytes, n_ctgs = self.contig_index_info()
        prm = _lib.kc_polish_params(min_score, min_len, edge_clip, max_mismatches, min_depth, min_permille, min_qual,
                                    _lib.KC_POLISH_BEST_ONLY if best_only else 0)
        st = _lib.kc_polish_stats()
        exact = with_fixes is not True and with_fixes is not False
        capacity = int(with_fixes) if exact else nbytes
        out = self._out(dev, nbytes, np.uint8, pad=True)
        counts = self._out(dev, nbytes * 4, np.uint16, pad=True) if with_counts else None
        recs = self._out(dev, n_ctgs, POLISH_CTG_DTYPE, pad=True) if with_records else None
        fixes = self._out(dev, capacity, POLISH_FIX_DTYPE, pad=True) if with_fixes is not False else None
        self._hand_over(dev)
        if not nb_reads:  # no bases at all: the library takes no byte arrays then
            pb = pq = None
        check(lib().kc_ctg_polish(self._h, pb, pq, po, nreads, pa, n_alns, 1 if dev else 0, C.byref(prm), out.ptr, counts and counts.ptr,
                                  recs and recs.ptr, fixes and fixes.ptr, capacity, C.byref(st)), "kc_ctg_polish")
        c = counts and counts.first()
        if c is not None and not dev:
            c = c.reshape(nbytes, 4)
        return out.first(), c, recs and recs.first(), fixes and fixes.first(int(st.changed)), _stats_dict(st)

    def polish_strings(self, bases, offsets, gap_alns, **kw):
        """polish_contigs' block as a host list of contig strings: for tests and small inputs."""
        return polish_strings(self, bases, offsets, gap_alns, **kw)

    def break_contigs(self, offsets, gap_alns, pairs, depths=None, max_insert=1000, max_span=0, min_disc=3, margin=None, min_run=1, one_mate=False,
                      tracks=False):
        """The indexed contigs cut where no read pair spans them and the mates that should have landed elsewhere (kc_ctg_break;
        DESIGN.md section 34).  offsets: the reads' starts (no bases are needed; reads 2p and 2p + 1 are mates); gap_alns
        align_gapped's records, pairs pair_inserts' records (their classes are not read: every pair is classified again);
        depths: one uint16 per byte of the indexed block, or None.  A pair on one contig, its mates facing each other at most
        max_insert apart, spans the columns between its outer ends; every other aligned mate is discordant over the max_insert
        columns in which its partner should have been (one_mate: also a mate whose partner has no record).  A column at least
        margin (None: max_insert) from both ends of its contig with at most max_span spanning pairs and at least min_disc
        discordant mates is weak; a run of min_run or more weak columns is cut in its middle.  Returns (seqs, offsets, depths
        or None, pieces, breaks, stats, tracks): the block index_contigs, submit_ctg_block, dedup_contigs, select_contigs and
        fasta_text take as it is, one BREAK_PIECE_DTYPE record per output contig, one BREAK_DTYPE record per break,
        kc_break_stats as a dict, and with tracks the pair (span, disc) of saturated uint16 counts over the input block (else
        None).  Host arrays in give numpy arrays out; device tensors in give device tensors out (offsets int64, depths and
        tracks int16, records uint8 tensors).  A size query comes first, so every array is exact."""
        pa, n_alns, dev_a = _records("gap_alns", gap_alns, GAP_ALN_DTYPE)
        pp, n_pairs, dev_p = _records("pairs", pairs, PAIR_DTYPE)
        po, dev_o = _ptr(offsets)
        nreads = len(offsets) - 1
        nbytes, n_ctgs = self.contig_index_info()
        nd = 0 if depths is None else (depths.numel() if _ptr(depths)[1] else len(depths))
        dev = _side("offsets", dev_o, gap_alns=(dev_a, n_alns), pairs=(dev_p, n_pairs), depths=(_ptr(depths)[1], nd))
        if n_pairs != nreads // 2:
            raise ValueError("pairs: one record per pair of reads")
        if depths is not None and nd != nbytes:
            raise ValueError("depths: one uint16 per byte of the indexed block")
        prm = _lib.kc_break_params(max_insert, max_span, min_disc, max_insert if margin is None else margin, min_run,
                                   _lib.KC_BREAK_ONE_MATE if one_mate else 0)
        st, no, nb = _lib.kc_break_stats(), C.c_uint64(0), C.c_uint64(0)
        head = (self._h, po, nreads, pa, n_alns, pp, _ptr(depths)[0], 1 if dev else 0, C.byref(prm))
        tail = (C.byref(no), C.byref(nb), C.byref(st))
        self._hand_over(dev)
        check(lib().kc_ctg_break(*head, None, 0, None, None, None, None, 0, None, None, *tail), "kc_ctg_break")
        n_out, total, n_brk = int(no.value), int(nb.value), int(st.breaks)
        seqs, offs_out = self._out(dev, total, np.uint8, pad=True), self._out(dev, n_out + 1, np.uint64)
        depths_out = None if depths is None else self._out(dev, total, np.uint16, pad=True)
        pieces, recs = self._out(dev, n_out, BREAK_PIECE_DTYPE, pad=True), self._out(dev, n_brk, BREAK_DTYPE, pad=True)
        tr = (self._out(dev, nbytes, np.uint16, pad=True), self._out(dev, nbytes, np.uint16, pad=True)) if tracks else None
        self._hand_over(dev)  # fresh arrays
        check(lib().kc_ctg_break(*head, seqs.ptr, total, offs_out.ptr, depths_out and depths_out.ptr, pieces.ptr, recs.ptr, n_brk,
                                 tr and tr[0].ptr, tr and tr[1].ptr, *tail), "kc_ctg_break")
        return (seqs.first(), offs_out.first(), depths_out and depths_out.first(), pieces.first(), recs.first(), _stats_dict(st),
                tr and (tr[0].first(), tr[1].first()))

    def break_strings(self, offsets, gap_alns, pairs, **kw):
        """break_contigs' block as a host list of contig strings: for tests and small inputs."""
        return break_strings(self, offsets, gap_alns, pairs, **kw)

    def contig_kmer_depths(self, seqs, offsets):
        """One depth per byte of a seq block, from the k-mer counts of the finished results: every contig's mean window count
        on its bases, 0 on its separator.  The array submit_ctg_block takes."""
        return self.kmer_depths(seqs, offsets, fill_mean=True, with_records=False)[0]

    def count_spectrum(self, on_device=False):
        """The histogram of the results' counts (kc_count_spectrum): (hist, stats), hist[c] the number of results whose count
        is c, a uint64 numpy array of 65536 values (on_device: an int64 device tensor), and kc_spectrum_stats as a dict."""
        hist = self._out(on_device, _lib.KC_SPECTRUM_BINS, np.uint64)
        st = _lib.kc_spectrum_stats()
        self._hand_over(on_device)
        check(lib().kc_count_spectrum(self._h, hist.ptr, 1 if on_device else 0, C.byref(st)), "kc_count_spectrum")
        return hist.first(), _stats_dict(st)

    def _fasta_call(self, seqs, offsets, order, prefix, line_width):
        """what the windows of one text share: call(first_byte, address, capacity) -> (written, total), and the side"""
        p_order, dev_o = _ptr(order)
        n_order = 0 if order is None else (order.numel() if dev_o else len(order))
        if order is not None and not dev_o and (order.dtype.itemsize != 4 or not order.flags["C_CONTIGUOUS"]):
            raise ValueError("order: a contiguous array of 32-bit indices")
        ps, nbytes, po, n, dev = self._block(seqs, offsets, order=(dev_o, n_order))
        prefix = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
        prm = _lib.kc_fasta_params(line_width, len(prefix), 0, 0, prefix[:_lib.KC_FASTA_MAX_PREFIX])
        if order is None:
            n_order = n

        def call(first_byte, text, capacity):
            written, total = C.c_uint64(0), C.c_uint64(0)
            if order is not None and not n_order:  # an empty selection: an empty text (an empty array has no address to pass)
                return 0, 0
            check(lib().kc_fasta_text(self._h, ps, nbytes, po, n, p_order, n_order, 1 if dev else 0, C.byref(prm), first_byte, text,
                                      capacity, C.byref(written), C.byref(total)), "kc_fasta_text")
            return int(written.value), int(total.value)

        return call, dev

    def fasta_text(self, seqs, offsets, order=None, prefix="scaffold_", line_width=0, first_byte=0, capacity=None):
        """The FASTA text of a seq block's contigs, formatted on the device (kc_fasta_text), as bytes:
        for every entry u of order (None: all contigs in block order; select_contigs' order as it comes) the record
        ">" prefix u "\\n" and the contig in lines of line_width bases (0: one line, dump_contigs' format).  first_byte /
        capacity: bytes [first_byte, first_byte + capacity) of the whole text only (capacity None: to its end)."""
        call, dev = self._fasta_call(seqs, offsets, order, prefix, line_width)
        self._hand_over(dev)
        _, total = call(first_byte, None, 0)
        want = total - first_byte if capacity is None else min(capacity, total - first_byte)
        if want <= 0:
            return b""
        text = self._out(dev, want, np.uint8)
        self._hand_over(dev)
        written, _ = call(first_byte, text.ptr, want)
        out = text.first(written)
        return (out.cpu().numpy() if dev else out).tobytes()

    def write_fasta(self, path_or_fileobj, seqs, offsets, order=None, prefix="scaffold_", line_width=0, window_bytes=256 << 20):
        """fasta_text() streamed to a file: the text goes through one buffer of window_bytes, window after window, each
        written to the file object (a path is opened "wb"; compression and the file itself stay with the caller's file
        object).  Returns the text's bytes.  The records' starts are recomputed for every window: keep windows large."""
        if window_bytes < 1:
            raise ValueError("window_bytes: at least 1")
        if isinstance(path_or_fileobj, (str, bytes)) or hasattr(path_or_fileobj, "__fspath__"):
            with open(path_or_fileobj, "wb") as f:
                return self.write_fasta(f, seqs, offsets, order, prefix, line_width, window_bytes)
        call, dev = self._fasta_call(seqs, offsets, order, prefix, line_width)
        self._hand_over(dev)
        _, total = call(0, None, 0)
        text = self._out(dev, min(window_bytes, total), np.uint8)
        self._hand_over(dev)
        first = 0
        while first < total:
            written, _ = call(first, text.ptr, text.n)
            out = text.first(written)
            path_or_fileobj.write((out.cpu().numpy() if dev else out).tobytes())
            first += written
        return total

    def _fastq_call(self, bases, quals, offsets, order, ids, prefix, paired, first_id, nreads):
        """what the windows of one FASTQ text share: call(first_byte, address, capacity, check) -> (written, total), and the side"""
        pb, dev_b = _ptr(bases)
        pq, dev_q = _ptr(quals)
        po, dev_o = _ptr(offsets)
        p_order, dev_r = _ptr(order)
        p_ids, dev_i = _ptr(ids)
        n = (len(offsets) - 1) if nreads is None else nreads
        n_order = n if order is None else (order.numel() if dev_r else len(order))
        if order is not None and not dev_r and (order.dtype.itemsize != 4 or not order.flags["C_CONTIGUOUS"]):
            raise ValueError("order: a contiguous array of 32-bit indices")
        if ids is not None and not dev_i and (ids.dtype.itemsize != 8 or not ids.flags["C_CONTIGUOUS"]):
            raise ValueError("ids: a contiguous array of 64-bit numbers")
        nbytes = bases.numel() if dev_b else len(bases)
        dev = _side("bases", dev_b, quals=(dev_q, 0 if quals is None else nbytes), offsets=(dev_o, True),
                    order=(dev_r, 0 if order is None else n_order), ids=(dev_i, 0 if ids is None else n))
        keep = None
        if quals is not None and not pq:  # reads without a byte: an empty array has no address, and NULL would mean packed
            keep = self._out(dev, 1, np.uint8, zeroed=True)
            pq = keep.ptr
        prefix = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
        flags = (_lib.KC_FASTQ_OUT_PACKED if quals is None else 0) | (_lib.KC_FASTQ_OUT_PAIRED if paired else 0)
        prm = _lib.kc_fastq_out_params(flags, len(prefix), first_id, prefix[:_lib.KC_FASTQ_OUT_MAX_PREFIX])

        def call(first_byte, text, capacity, check=False, _keep=keep):
            written, total = C.c_uint64(0), C.c_uint64(0)
            if order is not None and not n_order:  # an empty selection: an empty text (an empty array has no address to pass)
                return 0, 0
            prm.flags = flags | (_lib.KC_FASTQ_OUT_CHECK if check else 0)
            _lib.check(lib().kc_fastq_text(self._h, pb if nbytes else None, pq, po, n, p_order, n_order, p_ids, 1 if dev else 0, C.byref(prm),
                                           first_byte, text, capacity, C.byref(written), C.byref(total)), "kc_fastq_text")
            return int(written.value), int(total.value)

        return call, dev

    def fastq_text(self, bases, quals, offsets, order=None, ids=None, prefix="r", paired=False, first_id=0, check=False, first_byte=0,
                   capacity=None, nreads=None):
        """The FASTQ text of reads, formatted on the device (kc_fastq_text), as bytes: for every entry i
        of order (None: all reads) the record "@" prefix number "\\n" bases "\\n+\\n" qualities "\\n", number = ids[i], or
        first_id + i without ids.  bases / quals / offsets: the front end's layout, numpy arrays or device tensors;
        quals=None: bases holds packed reads (merge_pairs', fastq_to_packed's output).  paired: reads 2p and 2p+1 are mates,
        both numbered first_id + 2p, their names end in "/1" and "/2" (merge_reads' --dump-merged naming).  check: refuse
        bytes that would not parse back (KC_ERR_BAD_BASE).  first_byte / capacity: bytes [first_byte, first_byte + capacity)
        of the whole text only (capacity None: to its end)."""
        call, dev = self._fastq_call(bases, quals, offsets, order, ids, prefix, paired, first_id, nreads)
        self._hand_over(dev)
        _, total = call(first_byte, None, 0, check)
        want = total - first_byte if capacity is None else min(capacity, total - first_byte)
        if want <= 0:
            return b""
        text = self._out(dev, want, np.uint8)
        self._hand_over(dev)
        written, _ = call(first_byte, text.ptr, want)
        out = text.first(written)
        return (out.cpu().numpy() if dev else out).tobytes()

    def write_fastq(self, path_or_fileobj, bases, quals, offsets, order=None, ids=None, prefix="r", paired=False, first_id=0, check=False,
                    nreads=None, window_bytes=256 << 20):
        """fastq_text() streamed to a file: the text goes through one buffer of window_bytes, window after window, each
        written to the file object (a path is opened "wb"; compression and the file itself stay with the caller's file
        object).  check is made once, in front of the first window.  Returns the text's bytes.  The records' starts are
        recomputed for every window: keep windows large."""
        if window_bytes < 1:
            raise ValueError("window_bytes: at least 1")
        if isinstance(path_or_fileobj, (str, bytes)) or hasattr(path_or_fileobj, "__fspath__"):
            with open(path_or_fileobj, "wb") as f:
                return self.write_fastq(f, bases, quals, offsets, order, ids, prefix, paired, first_id, check, nreads, window_bytes)
        call, dev = self._fastq_call(bases, quals, offsets, order, ids, prefix, paired, first_id, nreads)
        self._hand_over(dev)
        _, total = call(0, None, 0, check)
        text = self._out(dev, min(window_bytes, total), np.uint8)
        self._hand_over(dev)
        first = 0
        while first < total:
            written, _ = call(first, text.ptr, text.n)
            out = text.first(written)
            path_or_fileobj.write((out.cpu().numpy() if dev else out).tobytes())
            first += written
        return total

    def write_fastq_pairs(self, path1, path2, bases, quals, offsets, ids=None, prefix="r", first_id=0, check=False, first_pair=0, npairs=None,
                          window_bytes=256 << 20):
        """Interleaved pairs as a pair of FASTQ files: mates 1 (the even reads) go to path1 and mates 2 to path2, both
        under the pair's number with "/1" and "/2" (write_fastq with paired=True and order = the even / the odd reads).
        first_pair / npairs: pairs [first_pair, first_pair + npairs) only (npairs None: to the last), so that one part of
        shuffle_reads (part_starts) goes to files of its own.  Returns both texts' bytes."""
        total_pairs = (len(offsets) - 1) // 2
        npairs = total_pairs - first_pair if npairs is None else npairs
        if first_pair < 0 or npairs < 0 or first_pair + npairs > total_pairs:
            raise ValueError("pairs [%d, %d) of %d" % (first_pair, first_pair + npairs, total_pairs))
        dev = _ptr(bases)[1]
        sizes = []
        for mate, path in enumerate((path1, path2)):
            order = np.arange(2 * first_pair + mate, 2 * (first_pair + npairs), 2, dtype=np.uint32)
            if dev:
                import torch
                order = torch.from_numpy(order.view(np.int32)).to(self._torch_device())
            sizes.append(self.write_fastq(path, bases, quals, offsets, order, ids, prefix, True, first_id, check, 2 * total_pairs, window_bytes))
        return tuple(sizes)

    def fasta_to_block(self, text, partial=False, strict=False, default_depth=0, with_depths=False, with_records=True):
        """FASTA text parsed on the device into a seq block (kc_fasta_to_block), the inverse of
        fasta_text: line-wrapped or not, lower case and IUPAC codes recoded (strict: refused), CRLF and trailing blanks
        stripped.  text: bytes, a numpy uint8 array (staged) or a uint8 device tensor (read in place); the result lies on
        the side the text came from.  Returns a dict: seqs (every contig followed by '_'), offsets (contigs + 1), depths
        (with_depths: one uint16 per byte, the header's depth or default_depth on the bases, what submit_ctg_block takes;
        else None), records (with_records: FASTA_REC_DTYPE per contig, a uint8 tensor of 32-byte records on the device; else
        None), consumed and stats.  partial: the text is a prefix of a longer one, only the records in front of its last
        header are parsed and `consumed` is that header's position; the caller carries the tail."""
        if not 0 <= default_depth <= 65535:
            raise ValueError("default_depth: 0 .. 65535")
        pt, n, dev, keep = _text(text)
        dev = _side("text", dev)
        prm = _lib.kc_fasta_in_params((_lib.KC_FASTA_PARTIAL if partial else 0) | (_lib.KC_FASTA_STRICT if strict else 0), default_depth)
        seqs = self._out(dev, n, np.uint8, pad=True)  # a header gives a byte and is one at least, a base gives one
        depths = self._out(dev, n, np.uint16, pad=True) if with_depths else None
        nc, nb, cons, st = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), _lib.kc_fasta_in_stats()

        def call(capacity):
            offs = self._out(dev, capacity + 1, np.uint64)
            recs = self._out(dev, capacity, FASTA_REC_DTYPE, pad=True) if with_records else None
            self._hand_over(dev)
            rc = lib().kc_fasta_to_block(self._h, pt, n, 1 if dev else 0, C.byref(prm), seqs.ptr, n, offs.ptr, capacity, depths and depths.ptr,
                                         recs and recs.ptr, C.byref(nc), C.byref(nb), C.byref(cons), C.byref(st))
            return rc, int(nc.value), (offs, recs)

        rc, _, (offs, recs) = _retry_on_capacity(n // 64 + 16, call)
        check(rc, "kc_fasta_to_block")
        del keep
        c, b = int(nc.value), int(nb.value)
        return {"seqs": seqs.first(b), "offsets": offs.first(c + 1), "depths": depths and depths.first(b), "records": recs and recs.first(c),
                "consumed": int(cons.value), "stats": _stats_dict(st)}

    def load_contigs(self, path_or_fileobj, window_bytes=256 << 20, strict=False, default_depth=0, with_depths=False, with_records=True):
        """fasta_to_block() streamed from a file (a path is opened "rb"; decompression stays with the caller's file
        object): the text goes through one device buffer of window_bytes with partial=True, the unfinished tail carried
        into the next window, the window doubled when it holds no whole record, the last call without the flag.  Returns
        fasta_to_block's dict for the whole file as device tensors: one block, the offsets rebased, hdr_pos as file
        positions, the stats summed (longest: the maximum), consumed the file's bytes.  An error in any window raises and
        returns nothing."""
        import torch
        if window_bytes < 1:
            raise ValueError("window_bytes: at least 1")
        if not 0 <= default_depth <= 65535:
            raise ValueError("default_depth: 0 .. 65535")
        if isinstance(path_or_fileobj, (str, bytes)) or hasattr(path_or_fileobj, "__fspath__"):
            with open(path_or_fileobj, "rb") as f:
                return self.load_contigs(f, window_bytes, strict, default_depth, with_depths, with_records)
        kw = dict(strict=strict, default_depth=default_depth, with_depths=with_depths, with_records=with_records)
        window = self._out(True, window_bytes, np.uint8)
        parts, stats, tail, pos, nbytes = [], None, b"", 0, 0  # pos: the file position of the window's first byte
        while True:
            while len(tail) >= window.n:  # a record longer than the window
                window = self._out(True, 2 * window.n, np.uint8)
            chunk = path_or_fileobj.read(window.n - len(tail))
            buf = bytearray(tail)  # (writable: torch takes no read-only memory)
            buf += chunk
            text = window.first(len(buf))
            if buf:
                text.copy_(torch.from_numpy(np.frombuffer(buf, dtype=np.uint8)))
            r = self.fasta_to_block(text, partial=bool(chunk), **kw)
            used = r["consumed"]
            if r["offsets"].numel() > 1:
                if with_records:
                    r["records"].view(torch.int64).view(-1, 4)[:, 0] += pos
                parts.append((r["seqs"], r["offsets"][1:] + nbytes, r["depths"], r["records"]))
                nbytes += r["seqs"].numel()
            st = r["stats"]
            stats = st if stats is None else {k: max(v, st[k]) if k == "longest" else v + st[k] for k, v in stats.items()}
            pos += used
            tail = buf[used:]
            if not chunk:
                break
        cat = lambda j, dtype: torch.cat([p[j] for p in parts]) if parts else torch.zeros(0, dtype=dtype, device=self._torch_device())  # noqa: E731
        zero = torch.zeros(1, dtype=torch.int64, device=self._torch_device())
        return {"seqs": cat(0, torch.uint8), "offsets": torch.cat([zero] + [p[1] for p in parts]), "depths": cat(2, torch.int16) if with_depths else None,
                "records": cat(3, torch.uint8) if with_records else None, "consumed": pos, "stats": stats}

    def submit_ctg_block(self, seqs, depths):
        """kc_submit_ctg_block with device tensors (a '_'-joined block and one 16-bit depth per byte), e.g. those of
        unitig_block(); begin_ctg_kmers first."""
        ps, dev = _ptr(seqs)
        pd, _ = _ptr(depths)
        if not dev:
            raise ValueError("submit_ctg_block takes device tensors; submit_ctgs is the host path")
        check(lib().kc_submit_ctg_block(self._h, ps, pd, seqs.numel(), 1), "kc_submit_ctg_block")

    def dump_kmers(self, directory=".", rank=None, on_device=False, chunk_lines=1 << 24):
        """KmerDHT::dump_kmers (src/kcount/kmer_dht.cpp:273-297): per-rank gzip text file "kmers-<k>.txt.gz", one
        "KMER count L R" line per k-mer.  Returns the path.  on_device=True: the results are sorted and formatted on
        the GPU and written chunk by chunk (chunk_lines lines at a time through dump_text); the default is the host
        path, sorted_results() and dump_lines()."""
        import gzip
        import os
        r = self.rank_me if rank is None else rank
        d = os.path.join(directory, "rank_%d" % r) if self.rank_n > 1 else directory
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "kmers-%d.txt.gz" % self.k)
        if on_device:
            n = int(self.sort_results().n)
            with gzip.open(path, "wb") as f:
                for first in range(0, n, chunk_lines):
                    f.write(self.dump_text(first, min(chunk_lines, n - first), sort=False))
            return path
        with gzip.open(path, "wt") as f:
            for line in self.dump_lines():
                f.write(line + "\n")
        return path


# a record of kc_align_reads (kc_read_aln): 32 bytes
ALN_DTYPE = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("cstart", "<u4"), ("cstop", "<u4"), ("rstart", "<u2"), ("rstop", "<u2"),
                      ("mismatches", "<u2"), ("seeds", "<u2"), ("orient", "u1"), ("pad", "u1", (7,))])


# a record of kc_align_gapped (kc_gap_aln): 32 bytes
GAP_ALN_DTYPE = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("cstart", "<u4"), ("cstop", "<u4"), ("rstart", "<u2"), ("rstop", "<u2"),
                          ("score", "<u4"), ("mismatches", "<u2"), ("seeds", "<u2"), ("orient", "u1"), ("kind", "u1"), ("pad", "u1", (2,))])
# match, mismatch, gap open, gap extend, ambiguity (CMakeDefinitions.txt:133-134)
# kc_aln_depths' record of a contig (kc_ctg_depth, 32 bytes) and kc_pair_inserts' record of a pair (kc_pair_rec, 16 bytes)
CTG_DEPTH_DTYPE = np.dtype([("depth_sum", "<u8"), ("len", "<u4"), ("covered", "<u4"), ("min_depth", "<u4"), ("max_depth", "<u4"),
                            ("alns", "<u4"), ("mean", "<u4")])
PAIR_DTYPE = np.dtype([("aln0", "<u4"), ("aln1", "<u4"), ("insert", "<u4"), ("cls", "u1"), ("pad", "u1", (3,))])
# kc_local_assm's record of a contig end (kc_lassm_end, 16 bytes)
LASSM_END_DTYPE = np.dtype([("cands", "<u4"), ("ext_len", "<u4"), ("out_pos", "<u4"), ("iters", "<u2"), ("mer_len", "u1"), ("status", "u1")])
LINK_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("splints", "<u4"), ("spans", "<u4"), ("splint_gap_min", "<i4"), ("splint_gap_max", "<i4"),
                       ("span_gap_min", "<i4"), ("span_gap_max", "<i4"), ("splint_gap_sum", "<i8"), ("span_gap_sum", "<i8")])
# kc_scaffold's records of a scaffold (kc_scaffold_rec, 32 bytes) and of a member (kc_scaf_member, 16 bytes)
SCAFFOLD_DTYPE = np.dtype([("first_member", "<u4"), ("n_members", "<u4"), ("len", "<u4"), ("n_bases", "<u4"), ("overlap_bases", "<u4"),
                           ("flags", "<u4"), ("pad", "<u4", (2,))])
MEMBER_DTYPE = np.dtype([("ctg", "<u4"), ("join", "<i4"), ("out_pos", "<u4"), ("orient", "u1"), ("pad", "u1", (3,))])
# kc_close_gaps' record of a member's join (kc_closure, 32 bytes)
CLOSURE_DTYPE = np.dtype([("cands", "<u4"), ("reads", "<u4"), ("old_join", "<i4"), ("new_join", "<i4"), ("fill_pos", "<u4"), ("disputed", "<u4"),
                          ("status", "u1"), ("pad", "u1", (3,)), ("reserved", "<u4")])
# kc_fasta_to_block's record of a contig (kc_fasta_rec, 32 bytes)
FASTA_REC_DTYPE = np.dtype([("hdr_pos", "<u8"), ("hdr_len", "<u4"), ("seq_lines", "<u4"), ("id", "<u8"), ("depth", "<u4"), ("flags", "<u4")])
# kc_ctg_dedup's record of an input contig (kc_dedup_rec, 32 bytes)
DEDUP_DTYPE = np.dtype([("status", "<u4"), ("container", "<u4"), ("pos", "<u4"), ("mismatches", "<u4"), ("new_index", "<u4"), ("len", "<u4"),
                        ("absorbed", "<u4"), ("orient", "u1"), ("flags", "u1"), ("pad", "u1", (2,))])
# kc_seq_kmer_depths' record of a sequence (kc_kdepth_rec, 32 bytes)
KDEPTH_DTYPE = np.dtype([("sum", "<u8"), ("windows", "<u4"), ("present", "<u4"), ("solid", "<u4"), ("min_count", "<u2"), ("max_count", "<u2"),
                         ("mean", "<u2"), ("pad", "<u2", (3,))])

# kc_correct_reads' record of a sequence (kc_correct_rec) and entry of a corrected byte (kc_correct_fix), 16 bytes each
CORRECT_REC_DTYPE = np.dtype([("weak_before", "<u4"), ("weak_after", "<u4"), ("corrected", "<u2"), ("flags", "<u2"), ("reserved", "<u4")])
CORRECT_FIX_DTYPE = np.dtype([("seq", "<u4"), ("pos", "<u4"), ("old", "u1"), ("new", "u1"), ("round", "u1"), ("side", "u1"), ("score", "<u2"),
                              ("runner_up", "<u2")])

# kc_ctg_polish's record of a contig (kc_polish_ctg, 32 bytes) and entry of a changed column (kc_polish_fix, 16 bytes)
POLISH_CTG_DTYPE = np.dtype([("votes", "<u8"), ("placed", "<u4"), ("changed", "<u4"), ("filled", "<u4"), ("disputed", "<u4"), ("thin", "<u4"),
                             ("uncovered", "<u4")])
POLISH_FIX_DTYPE = np.dtype([("pos", "<u4"), ("ctg", "<u4"), ("old", "u1"), ("new", "u1"), ("top", "<u2"), ("tot", "<u2"), ("pad", "<u2")])


def polish_strings(kc, bases, offsets, gap_alns, **kw):
    """kc.polish_contigs(...)'s block as a host list of contig strings, in the index's order: for tests and small inputs."""
    block = kc.polish_contigs(bases, offsets, gap_alns, with_records=False, with_fixes=False, **kw)[0]
    text = (block if isinstance(block, np.ndarray) else block.cpu().numpy()).tobytes().decode()
    return text.split("_")[:-1]


# kc_ctg_break's record of an output contig (kc_break_piece, 16 bytes) and of a break (kc_break_rec, 32 bytes)
BREAK_PIECE_DTYPE = np.dtype([("ctg", "<u4"), ("start", "<u4"), ("len", "<u4"), ("flags", "<u4")])
BREAK_DTYPE = np.dtype([("ctg", "<u4"), ("pos", "<u4"), ("run_start", "<u4"), ("run_len", "<u4"), ("span", "<u4"), ("disc", "<u4"), ("piece", "<u4"),
                        ("pad", "<u4")])


def break_strings(kc, offsets, gap_alns, pairs, **kw):
    """kc.break_contigs(...)'s block as a host list of contig strings, in block order: for tests and small inputs."""
    return _block_strings(*kc.break_contigs(offsets, gap_alns, pairs, **kw)[:2])


def format_spectrum(hist):
    """The text of a count spectrum: a line "<count> <kmers>\n" for every bin that is not zero, counts ascending.  hist: what
    count_spectrum returns, a numpy array or a device tensor."""
    if not isinstance(hist, np.ndarray):
        hist = hist.cpu().numpy()
    hist = np.ascontiguousarray(hist).view(np.uint64)  # a tensor's int64 holds the bits
    return "".join("%d %d\n" % (c, int(hist[c])) for c in np.flatnonzero(hist))


BLASTN_ALN_SCORES = (2, 3, 5, 2, 1)
ALTERNATE_ALN_SCORES = (1, 1, 1, 1, 1)


def format_assembly_stats(stats, min_len):
    """The few lines print_stats(min_ctg_len) would log, from select_contigs' stats."""
    tot = max(stats["sel_bases"], 1)
    lines = ["Assembly statistics (contig lengths >= %d)" % min_len,
             "    Number of contigs:       %d" % stats["selected"],
             "    Total assembled length:  %d" % stats["sel_bases"],
             "    Number of Ns/100kbp:     %.2f (%d)" % (stats["n"] * 100000.0 / tot, stats["n"]),
             "    Runs of Ns:              %d" % stats["n_runs"],
             "    Max. contig length:      %d" % stats["longest"],
             "    Min. contig length:      %d" % stats["shortest"],
             "    N50 / L50:               %d / %d" % (stats["n50"], stats["l50"]),
             "    N90 / L90:               %d / %d" % (stats["n90"], stats["l90"]),
             "    Contig lengths:"]
    for c, n, b in zip(_lib.KC_ASM_CLASSES, stats["ge_count"], stats["ge_bases"]):
        lines.append("        >= %-7d %10d contigs %14d bases (%.1f%%)" % (c, n, b, 100.0 * b / tot))
    return "\n".join(lines) + "\n"


def kmer_to_string(words, k):
    return "".join("ACGT"[(int(words[i // 32]) >> (2 * (31 - (i % 32)))) & 3] for i in range(k))


def fastq_to_packed(text, qual_offset=33):
    """FASTQ text (bytes) -> (packed u8, offsets u64): the read cache's bytes of src/packed_reads.cpp:99-126, ready for
    KmerCounter.submit_packed_reads.  Host only (FastqReader::get_next_fq_record's unpaired pass, src/fastq.cpp:1028+)."""
    data = text.encode() if isinstance(text, str) else bytes(text)
    n, nb = C.c_uint64(0), C.c_uint64(0)
    st = lib().kc_fastq_to_packed(data, len(data), qual_offset, None, 0, None, 0, C.byref(n), C.byref(nb))
    if st not in (_lib.KC_OK, _lib.KC_ERR_CAPACITY):
        check(st, "kc_fastq_to_packed")
    packed = np.zeros(max(nb.value, 1), dtype=np.uint8)
    offs = np.zeros(n.value + 1, dtype=np.uint64)
    check(lib().kc_fastq_to_packed(data, len(data), qual_offset, packed.ctypes.data, nb.value, offs.ctypes.data, n.value, C.byref(n),
                                   C.byref(nb)), "kc_fastq_to_packed")
    return packed[:nb.value], offs


def _adapter_text(text_or_path):
    if isinstance(text_or_path, str):
        with open(text_or_path, "rb") as f:
            return f.read()
    return bytes(text_or_path)


def adapters_index(text, adapter_k):
    """Adapter FASTA text (bytes) -> the loader's counts (kc_adapters_index, host only): kept sequences, sequences
    shorter than adapter_k, entries (both orientations) and distinct k-mers."""
    data = _adapter_text(text)
    return _adapter_counts("kc_adapters_index", data, len(data), adapter_k)


def fastq_pairs(text1, text2=None):
    """Paired FASTQ text (bytes; text2 None = text1 interleaved) -> interleaved ASCII (bases u8, quals u8, offsets u64), the
    input of KmerCounter.merge_pairs (kc_fastq_pairs, host only)."""
    t1 = text1.encode() if isinstance(text1, str) else bytes(text1)
    t2 = None if text2 is None else (text2.encode() if isinstance(text2, str) else bytes(text2))
    l2 = 0 if t2 is None else len(t2)
    n, nb = C.c_uint64(0), C.c_uint64(0)
    st = lib().kc_fastq_pairs(t1, len(t1), t2, l2, None, None, 0, None, 0, C.byref(n), C.byref(nb))
    if st not in (_lib.KC_OK, _lib.KC_ERR_CAPACITY):
        check(st, "kc_fastq_pairs")
    bases = np.zeros(max(nb.value, 1), dtype=np.uint8)
    quals = np.zeros(max(nb.value, 1), dtype=np.uint8)
    offs = np.zeros(n.value + 1, dtype=np.uint64)
    check(lib().kc_fastq_pairs(t1, len(t1), t2, l2, bases.ctypes.data, quals.ctypes.data, nb.value, offs.ctypes.data, n.value,
                               C.byref(n), C.byref(nb)), "kc_fastq_pairs")
    return bases[:nb.value], quals[:nb.value], offs


def _count_and_sort(kc):
    """the end of every analyze_kmers flow: flush, then the sorted results and the counter's stats"""
    kc.flush()
    res = kc.sorted_results()
    return res, kc.stats()


def _merge_and_count(kc, bases, quals, offsets, min_kmer_len, adapters, blastn_scores, adapter_k):
    """the paired flows from interleaved reads on: trim where there are adapters, merge, submit the packed reads, count"""
    tst = None
    if adapters is not None:
        kc.load_adapters(adapters, adapter_k or min_kmer_len, blastn_scores)
        bases, quals, offsets, tst = kc.trim_adapters(bases, quals, offsets, paired=True)
    packed, offs, mst = kc.merge_pairs(bases, quals, offsets, min_kmer_len=min_kmer_len)
    if tst is not None:
        mst["trim"] = tst
    kc.submit_packed_reads(packed, offs, nreads=mst["out_reads"])
    return _count_and_sort(kc) + (mst,)


def analyze_kmers_paired(kmer_len, qual_offset, bases, quals, offsets, dmin_thres=2, device=0, max_elems=0, tuning=None,
                         min_kmer_len=0, adapters=None, blastn_scores=False, adapter_k=0):
    """merge_reads' pair loop then analyze_kmers for one shard: interleaved pairs are merged on the device
    (kc_merge_pairs), the merged read cache is counted (kc_submit_packed_reads).  Returns sorted results, the counter's
    stats and the merge's counters.  adapters (FASTA bytes, or a path as str): the pairs are adapter-trimmed on the
    device first (kc_trim_adapters) with k-mers of adapter_k (0: min_kmer_len, else kmer_len), and the merge's
    counters carry the trim's under "trim"."""
    with KmerCounter(kmer_len, qual_offset, dmin_thres, device=device, max_elems=max_elems, tuning=tuning) as kc:
        return _merge_and_count(kc, bases, quals, offsets, min_kmer_len, adapters, blastn_scores, adapter_k)


def analyze_kmers_fastq(kmer_len, qual_offset, text, dmin_thres=2, device=0, max_elems=0, tuning=None):
    """analyze_kmers from FASTQ text: parsed on the device (kc_fastq_to_packed_device), then counted.  Returns sorted
    results and stats."""
    with KmerCounter(kmer_len, qual_offset, dmin_thres, device=device, max_elems=max_elems, tuning=tuning) as kc:
        packed, offs = kc.fastq_to_packed(text)
        kc.submit_packed_reads(packed, offs, nreads=offs.numel() - 1)
        return _count_and_sort(kc)


def analyze_kmers_fastq_paired(kmer_len, qual_offset, text1, text2=None, dmin_thres=2, device=0, max_elems=0, tuning=None,
                               min_kmer_len=0, adapters=None, blastn_scores=False, adapter_k=0):
    """analyze_kmers_paired from paired FASTQ text (text2 None = text1 interleaved): parsed on the device
    (kc_fastq_pairs_device), merged (kc_merge_pairs), counted.  Returns sorted results, stats and the merge's counters.
    adapters: as for analyze_kmers_paired -- parse, trim (kc_trim_adapters), merge and count, all in device memory."""
    with KmerCounter(kmer_len, qual_offset, dmin_thres, device=device, max_elems=max_elems, tuning=tuning) as kc:
        bases, quals, offs = kc.fastq_pairs(text1, text2)
        return _merge_and_count(kc, bases, quals, offs, min_kmer_len, adapters, blastn_scores, adapter_k)


def analyze_kmers(kmer_len, qual_offset, bases, quals, offsets, dmin_thres=2, device=0, max_elems=0, tuning=None):
    """analyze_kmers (src/kcount/kcount.cpp:142-161) for one shard: returns sorted results and stats."""
    with KmerCounter(kmer_len, qual_offset, dmin_thres, device=device, max_elems=max_elems, tuning=tuning) as kc:
        kc.submit_reads(bases, quals, offsets)
        return _count_and_sort(kc)
