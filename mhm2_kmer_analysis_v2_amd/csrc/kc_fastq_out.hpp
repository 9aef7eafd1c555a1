// kc_fastq_out.hpp -- reads as FASTQ text on the device (kc_fastq_text): the inverse of the parsers of kc_fastq.hpp and
// the read side's twin of kc_fasta_text (kc_asm.hpp).  It plays the role of merge_reads' --dump-merged hand-over,
// src/merge_reads.cpp:335-340,379-382,635-647 of the reference: '@' name '\n' sequence '\n' '+' '\n' qualities '\n'.  The
// reference also writes " #<original name>" behind the name; this library keeps no names, so the rules are this
// project's own (pinned byte for byte by tests/fastq_out_model.py).  include/kcount_mi355.h states
// them in full.
//
// Kernels, in the order of the call:
//  kc_rtext_check_kernel   a thread per offset and per order entry: offsets that start at 0 and do not decrease, a read of
//                          2^32 bytes or more, the lowest entry of order that names no read, the lowest whose number has
//                          more than sixteen digits; with KC_FASTQ_OUT_CHECK and an order, the lowest entry that names
//                          each read.
//  kc_rtext_bytes_kernel   KC_FASTQ_OUT_CHECK only, input-centric: a thread per ALIGNED 16 bytes of a source array tests
//                          them in four words; only a thread that holds a bad byte searches the offsets for its read.
//                          The lowest order entry with a bad byte, by one atomicMin.
//  kc_rtext_detail_kernel  after a bad byte only, one workgroup over that entry's read: the first bad byte, bases before
//                          qualities.
//  kc_rtext_sizes_kernel   a thread per record: its bytes.
//  kc_link_tile_scan_kernel / kc_scan_kernel<1>, kc_rtext_starts_kernel  the records' 64-bit starts and the total.
//  kc_asm_spans_kernel     (kc_asm.hpp) the record that holds every 4096th byte of the window.
//  kc_rtext_write_kernel   the hot path, output-centric: a thread per ALIGNED 16 bytes of `text`.  The span table bounds
//                          a workgroup's records, a thread finds its record by a search of the starts.  A chunk inside a
//                          base line or a quality line is two aligned 16-byte loads of the source and a funnel shift
//                          (shuf_load16, kc_shuffle.hpp).  Every other chunk -- the "\n+\n" between the two lines, a
//                          record's end, a name line, an end of the window -- is built record by record: either line's
//                          bytes come out of sixteen bytes loaded from where the chunk would lie in that line, under the
//                          byte mask of the places at which the record's parts begin among the chunk's bytes; the three
//                          bytes and the last newline are constants under theirs; the name line is formed byte by
//                          byte, and so is a line whose aligned loads would leave the source.  Packed reads are decoded
//                          on the four words: the base by a byte permute out of the five letters, the quality by a
//                          shift, a mask and a carry-free add of the splat offset.  Whole chunks leave as one 16-byte
//                          store.
//
// No workgroup waits for another; every loop's trip count comes from the input (a search's steps, the records a chunk
// spans, a number's digits).
#pragma once
#include "kc_asm.hpp"

namespace kc {

constexpr int RTEXT_TPB = ASM_TPB;
constexpr int RTEXT_MAX_PREFIX = 32;
constexpr uint64_t RTEXT_MAX_NUMBER = 9999999999999999ull;  // sixteen digits: what a 64-bit BCD word carries

// the status words; the RT_BAD_* from RT_BAD_ORDER on start as all ones
enum { RT_BAD_OFFSETS = 0, RT_TOO_LONG, RT_TOTAL, RT_BAD_ORDER, RT_BAD_NUMBER, RT_BAD_J, RT_BAD_KEY, RT_BAD_BYTE, RT_BAD_READ, RT_COUNT };

struct RtextArgs {
  const uint8_t *bases;   // ASCII, or the read cache's packed bytes (quals null)
  const uint8_t *quals;
  uint64_t nbytes;        // offs[nreads]
  const uint64_t *offs;   // the nreads + 1 starts
  uint64_t nreads;
  const uint32_t *order;  // null: the identity
  uint64_t n_order;
  const uint64_t *ids;    // null: first_id + the read's index, or its pair's first
  uint64_t first_id;
  uint32_t *first_j;      // [nreads] the lowest order entry that names the read (KC_FASTQ_OUT_CHECK with an order)
  uint64_t *rs;           // [n_order + 1] the records' bytes, then their starts; the last is the total
  uint64_t *rbase;        // [tiles]
  const uint32_t *tab;    // the record that holds byte first_byte + 4096 w
  const uint8_t *prefix;  // prefix_len bytes in device memory
  uint32_t prefix_len;
  uint32_t paired;        // 1: "/1" and "/2" behind the number
  uint32_t qual_splat;    // the context's qual_offset in every byte
  uint64_t first_byte, written;
  uint8_t *text;
  uint64_t *st;
};

__device__ __forceinline__ uint32_t rtext_read_of(const RtextArgs &a, uint64_t j) { return a.order ? a.order[j] : (uint32_t)j; }

// the number in a read's name; all ones where first_id alone is too large (the sum cannot wrap then)
__device__ __forceinline__ uint64_t rtext_number(const RtextArgs &a, uint32_t i) {
  if (a.ids) return a.ids[i];
  return a.first_id > RTEXT_MAX_NUMBER ? ~0ull : a.first_id + (a.paired ? i & ~1u : i);
}

// Every offset is compared with its neighbour only; no byte of the reads is touched.
__global__ void __launch_bounds__(RTEXT_TPB) kc_rtext_check_kernel(RtextArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * RTEXT_TPB + threadIdx.x;
  if (a.nreads && t <= a.nreads) {
    const uint64_t o = a.offs[t];
    if (t == 0 && o != 0) a.st[RT_BAD_OFFSETS] = 1;
    if (t < a.nreads) {
      const uint64_t nxt = a.offs[t + 1];
      if (nxt < o)
        a.st[RT_BAD_OFFSETS] = 1;
      else if (nxt - o >= (1ull << 32))
        a.st[RT_TOO_LONG] = 1;
    }
  }
  if (t < a.n_order) {
    const uint32_t i = rtext_read_of(a, t);
    if (i >= a.nreads)
      atomicMin((unsigned long long *)&a.st[RT_BAD_ORDER], (unsigned long long)t);
    else {
      if (rtext_number(a, i) > RTEXT_MAX_NUMBER) atomicMin((unsigned long long *)&a.st[RT_BAD_NUMBER], (unsigned long long)t);
      if (a.first_j) atomicMin(&a.first_j[i], (uint32_t)t);
    }
  }
}

// 0x80 in every byte of w that a FASTQ line cannot hold (outside 0x21 .. 0x7E); packed: whose code is over 4
__device__ __forceinline__ uint32_t rtext_bad_bytes(uint32_t w, bool packed) {
  if (packed) return (((w & 0x07070707u) + 0x03030303u) & 0x08080808u) << 4;
  const uint32_t t = w & 0x7F7F7F7Fu;
  return (w | ~(t + 0x5F5F5F5Fu) | (t + 0x01010101u)) & 0x80808080u;
}

__device__ __forceinline__ bool rtext_bad_byte(uint32_t b, bool packed) { return packed ? (b & 7u) > 4u : b < 0x21u || b > 0x7Eu; }

// Thread t of array y (0 the bases, 1 the qualities) owns src[16 t - mis, 16 t - mis + 16) cut to [0, nbytes): mis = src's
// address & 15, so a whole chunk is one aligned 16-byte load.  The offsets and the order are valid; nbytes >= 1.
__global__ void __launch_bounds__(RTEXT_TPB) kc_rtext_bytes_kernel(RtextArgs a) {
  const bool packed = a.quals == nullptr;
  const uint8_t *src = blockIdx.y ? a.quals : a.bases;
  const uint64_t mis = (uint64_t)((uintptr_t)src & 15u);
  const int64_t p0 = (int64_t)(((uint64_t)blockIdx.x * RTEXT_TPB + threadIdx.x) * 16) - (int64_t)mis;
  if (p0 >= (int64_t)a.nbytes) return;
  const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < a.nbytes ? (uint64_t)(p0 + 16) : a.nbytes;
  uint32_t bad = 0;  // bit k: byte p0 + k
  if (to - from == 16) {
    const uint4 x = *(const uint4 *)(src + p0);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t m = rtext_bad_bytes(w[k], packed);
      bad |= (((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u)) << (4 * k);
    }
  } else {
    for (uint64_t p = from; p < to; p++) bad |= (rtext_bad_byte(src[p], packed) ? 1u : 0u) << (uint32_t)(p - (uint64_t)p0);
  }
  if (!bad) return;
  // the reads of the bad bytes: a search for the first, steps from there (empty reads are stepped over)
  uint64_t r = find_le(a.offs, (uint64_t)0, a.nreads - 1, (uint64_t)(p0 + (int64_t)__builtin_ctz(bad)));
  uint64_t best = ~0ull;
  while (bad) {
    const uint64_t p = (uint64_t)(p0 + (int64_t)__builtin_ctz(bad));
    bad &= bad - 1u;
    while (a.offs[r + 1] <= p) r++;  // ends: offs[nreads] = nbytes > p
    const uint64_t j = a.order ? (a.first_j[r] == 0xFFFFFFFFu ? ~0ull : (uint64_t)a.first_j[r]) : r;
    best = j < best ? j : best;
  }
  if (best != ~0ull) atomicMin((unsigned long long *)&a.st[RT_BAD_J], (unsigned long long)best);
}

// One workgroup over the read of order entry j: st[RT_BAD_KEY] = (1 for a quality, 0 for a base) << 32 | position of the
// first bad byte, st[RT_BAD_BYTE] = the byte, st[RT_BAD_READ] = the read.
__global__ void __launch_bounds__(RTEXT_TPB) kc_rtext_detail_kernel(RtextArgs a, uint64_t j) {
  __shared__ unsigned long long first;
  const bool packed = a.quals == nullptr;
  const uint32_t i = rtext_read_of(a, j);
  const uint64_t src = a.offs[i], len = a.offs[i + 1] - src;
  if (threadIdx.x == 0) first = ~0ull;
  __syncthreads();
  unsigned long long mine = ~0ull;
  for (uint64_t x = threadIdx.x; x < (packed ? len : 2 * len) && mine == ~0ull; x += RTEXT_TPB) {
    const bool q = x >= len;
    const uint64_t pos = q ? x - len : x;
    if (rtext_bad_byte((q ? a.quals : a.bases)[src + pos], packed)) mine = ((unsigned long long)q << 32) | pos;
  }
  if (mine != ~0ull) atomicMin(&first, mine);
  __syncthreads();
  if (threadIdx.x == 0 && first != ~0ull) {
    a.st[RT_BAD_KEY] = first;
    a.st[RT_BAD_READ] = i;
    a.st[RT_BAD_BYTE] = ((first >> 32) ? a.quals : a.bases)[src + (first & 0xFFFFFFFFull)];
  }
}

// the offsets, the order and the numbers are valid from here on
__global__ void __launch_bounds__(RTEXT_TPB) kc_rtext_sizes_kernel(RtextArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * RTEXT_TPB + threadIdx.x;
  if (j >= a.n_order) return;
  const uint32_t i = rtext_read_of(a, j);
  const uint64_t len = a.offs[i + 1] - a.offs[i];
  a.rs[j] = 6 + a.prefix_len + dec_digits<16>(rtext_number(a, i)) + 2 * a.paired + 2 * len;
}

// a.rs, a.rbase: scanned; a.st[RT_TOTAL] the total
__global__ void __launch_bounds__(RTEXT_TPB) kc_rtext_starts_kernel(RtextArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * RTEXT_TPB + threadIdx.x;
  if (j > a.n_order) return;
  a.rs[j] = j < a.n_order ? a.rbase[j >> LINK_SCAN_SHIFT] + a.rs[j] : a.st[RT_TOTAL];
}

// A record's bytes are [0, hdr) the name line, [hdr, mid) the bases, [mid, mid + 3) "\n+\n", [mid + 3, last) the qualities
// and `last` the final newline.
struct RtextRec {
  uint64_t start, end, src;  // the record's bytes in the text; the read's first byte in the source
  uint64_t mid, last;
  uint32_t i, hdr;
};

__device__ __forceinline__ RtextRec rtext_rec(const RtextArgs &a, uint64_t j) {
  RtextRec r;
  r.i = rtext_read_of(a, j);
  r.src = a.offs[r.i];
  const uint64_t len = a.offs[r.i + 1] - r.src;
  r.start = a.rs[j];
  r.end = a.rs[j + 1];
  r.hdr = (uint32_t)(r.end - r.start - 2 * len - 4);
  r.mid = r.hdr + len;
  r.last = r.mid + 3 + len;
  return r;
}

// four packed bytes as their letters: the code picks one of eight bytes, "ACGT" and four times 'N'
__device__ __forceinline__ uint32_t rtext_letters(uint32_t w) { return __builtin_amdgcn_perm(0x4E4E4E4Eu, 0x54474341u, w & 0x07070707u); }

// ... as their qualities: five bits and the offset, byte by byte without a carry into the neighbour
__device__ __forceinline__ uint32_t rtext_quals(uint32_t w, uint32_t splat) {
  const uint32_t q = (w >> 3) & 0x1F1F1F1Fu;
  return (q + (splat & 0x7F7F7F7Fu)) ^ (splat & 0x80808080u);
}

// the bytes of word k of a chunk whose index in the chunk is below c
__device__ __forceinline__ uint32_t rtext_below(int k, int c) {
  const int nb = c - 4 * k;
  return nb >= 4 ? 0xFFFFFFFFu : nb <= 0 ? 0u : (1u << (8 * nb)) - 1u;
}

// a record's part begins at byte x of the text: where that is among a chunk's sixteen bytes, 0 in front of them, 16 behind
__device__ __forceinline__ int rtext_clip(int64_t x) { return x < 0 ? 0 : x > 16 ? 16 : (int)x; }

// Thread t owns text[16 t - mis, 16 t - mis + 16) cut to [0, written): mis = text's address & 15, so every whole chunk is
// an aligned 16-byte store.  Byte x of `text` is byte first_byte + x of the whole.  n_order >= 1 and written >= 1.
__global__ void __launch_bounds__(RTEXT_TPB) kc_rtext_write_kernel(RtextArgs a) {
  const int tid = threadIdx.x;
  uint8_t *dst = a.text;
  const bool packed = a.quals == nullptr;
  const uint64_t mis = (uint64_t)((uintptr_t)dst & 15u);
  const uint64_t t0 = (uint64_t)blockIdx.x * RTEXT_TPB;
  if (t0 * 16 >= a.written + mis) return;
  // the records of the workgroup's first and last byte lie between those of the table's spans around them
  const uint64_t wg_first = t0 * 16 > mis ? t0 * 16 - mis : 0, wg_end = (t0 + RTEXT_TPB) * 16 - mis;
  const uint64_t w1 = (((wg_end < a.written ? wg_end : a.written) - 1) >> ASM_SPAN_SHIFT) + 1;
  const uint64_t lo = a.tab[wg_first >> ASM_SPAN_SHIFT];
  const uint64_t hi = (w1 << ASM_SPAN_SHIFT) < a.written ? (uint64_t)a.tab[w1] : a.n_order - 1;
  const int64_t p0 = (int64_t)((t0 + tid) * 16) - (int64_t)mis;
  if (p0 >= (int64_t)a.written) return;
  const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < a.written ? (uint64_t)(p0 + 16) : a.written;
  uint64_t j = find_le(a.rs, lo, hi, a.first_byte + from);
  RtextRec r = rtext_rec(a, j);
  const uint64_t q0 = a.first_byte + from - r.start;  // the first byte's place in its record
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const bool whole = to - from == 16;
  const uintptr_t b_lo = (uintptr_t)a.bases, q_lo = packed ? b_lo : (uintptr_t)a.quals;
  bool done = false;
  if (whole && q0 >= r.hdr && q0 + 16 <= r.mid) {  // inside the base line
    done = shuf_load16(b_lo, b_lo + a.nbytes, b_lo + r.src + (q0 - r.hdr), w);
    if (done && packed) {
#pragma unroll
      for (int k = 0; k < 4; k++) w[k] = rtext_letters(w[k]);
    }
  } else if (whole && q0 >= r.mid + 3 && q0 + 16 <= r.last) {  // inside the quality line
    done = shuf_load16(q_lo, q_lo + a.nbytes, q_lo + r.src + (q0 - r.mid - 3), w);
    if (done && packed) {
#pragma unroll
      for (int k = 0; k < 4; k++) w[k] = rtext_quals(w[k], a.qual_splat);
    }
  }
  if (!done) {
    // Every other chunk, record by record (at most four: a record has seven bytes or more).  s0 .. s5: where among the
    // chunk's bytes the record, its bases, the three bytes between the lines, its qualities, its last newline and the next
    // record begin.  Either line comes out of sixteen bytes loaded from where the chunk would lie in it -- in front of
    // the read or behind it where the chunk holds other bytes there, which the masks drop -- and byte by byte where such
    // a load would leave the source; the name line is formed byte by byte.
    w[0] = w[1] = w[2] = w[3] = 0u;
    const int64_t g0 = (int64_t)a.first_byte + p0;
    const uint64_t g_end = a.first_byte + to;
    for (;;) {
      const int64_t d = (int64_t)r.start - g0, d_mid = d + (int64_t)r.mid, d_last = d + (int64_t)r.last;
      const int s0 = rtext_clip(d), s1 = rtext_clip(d + (int64_t)r.hdr), s2 = rtext_clip(d_mid), s3 = rtext_clip(d_mid + 3), s4 = rtext_clip(d_last),
                s5 = rtext_clip(d_last + 1);
      if (s1 > s0) {
        const uint64_t bcd = dec_bcd(rtext_number(a, r.i));
        const uint32_t sfx = 2u * a.paired;
#pragma unroll
        for (int k = 0; k < 16; k++) {
          if (k >= s0 && k < s1) {
            const uint32_t h = (uint32_t)((int64_t)k - d), tail = r.hdr - 1u - h;  // tail: bytes between this one and the newline
            const uint32_t ch = h == 0 ? (uint32_t)'@'
                              : h <= a.prefix_len ? (uint32_t)a.prefix[h - 1]
                              : tail == 0 ? (uint32_t)'\n'
                              : tail > sfx ? (uint32_t)'0' + (uint32_t)((bcd >> (4u * (tail - sfx - 1u))) & 15u)
                              : tail == 2 ? (uint32_t)'/'
                                          : (uint32_t)'1' + (r.i & 1u);
            w[k >> 2] |= ch << (8 * (k & 3));
          }
        }
      }
      if (s2 > s1) {
        uint32_t v[4];
        const int64_t at = -(d + (int64_t)r.hdr);  // the base at the chunk's byte 0
        if (shuf_load16(b_lo, b_lo + a.nbytes, b_lo + r.src + (uintptr_t)at, v)) {
#pragma unroll
          for (int k = 0; k < 4; k++) w[k] |= (packed ? rtext_letters(v[k]) : v[k]) & rtext_below(k, s2) & ~rtext_below(k, s1);
        } else {
#pragma unroll
          for (int k = 0; k < 16; k++) {
            if (k >= s1 && k < s2) {
              const uint32_t b = a.bases[r.src + (uint64_t)(at + k)];
              w[k >> 2] |= (packed ? (uint32_t)(0x4E4E4E4E54474341ull >> (8u * (b & 7u))) & 0xFFu : b) << (8 * (k & 3));
            }
          }
        }
      }
      if (s4 > s3) {
        uint32_t v[4];
        const int64_t at = -(d_mid + 3);  // the quality at the chunk's byte 0
        if (shuf_load16(q_lo, q_lo + a.nbytes, q_lo + r.src + (uintptr_t)at, v)) {
#pragma unroll
          for (int k = 0; k < 4; k++) w[k] |= (packed ? rtext_quals(v[k], a.qual_splat) : v[k]) & rtext_below(k, s4) & ~rtext_below(k, s3);
        } else {
#pragma unroll
          for (int k = 0; k < 16; k++) {
            if (k >= s3 && k < s4) {
              const uint32_t b = packed ? a.bases[r.src + (uint64_t)(at + k)] : a.quals[r.src + (uint64_t)(at + k)];
              w[k >> 2] |= (packed ? ((b >> 3) + a.qual_splat) & 0xFFu : b) << (8 * (k & 3));
            }
          }
        }
      }
      if (s3 > s2 || s5 > s4) {
        const int sm = d_mid < -3 ? -3 : d_mid > 19 ? 19 : (int)d_mid;  // where "\n+\n" begins, as far as a word can tell
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int s = sm - 4 * k;
          const uint32_t sep = s >= 4 || s <= -3 ? 0u : s >= 0 ? (uint32_t)(0x0A2B0Aull << (8 * s)) : 0x0A2B0Au >> (8 * -s);
          w[k] |= (sep & rtext_below(k, s3) & ~rtext_below(k, s2)) | (0x0A0A0A0Au & rtext_below(k, s5) & ~rtext_below(k, s4));
        }
      }
      if (r.end >= g_end) break;  // ends: rs[n_order] = the total >= g_end
      j++;
      r = rtext_rec(a, j);
    }
  }
  if (whole)
    *(uint4 *)(dst + p0) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int64_t p = p0 + k;
      if (p >= (int64_t)from && p < (int64_t)to) dst[p] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
  }
}

}  // namespace kc
