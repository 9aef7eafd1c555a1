// kc_asm.hpp -- the end of the assembly: which contigs are printed, in which order, the figures everybody quotes, and the
// FASTA text (kc_ctg_select, kc_fasta_text): the roles of ctgs.dump_contigs(fname, min_ctg_print_len, prefix),
// src/main.cpp:262 and src/contigging.cpp:115,180, and of ctgs.print_stats(min_ctg_len), src/contigging.cpp:184 and
// src/main.cpp:266, all commented out in the proxy.  The reference holds no Contigs class, so the rules are this
// project's own definition (pinned statement by statement by tests/asm_model.py); no parity with
// MetaHipMer is claimed.  include/kcount_mi355.h states the rules in full.
//
// Kernels of kc_ctg_select, in the order of the call (the check in front of them is kc_align_check_kernel):
//  kc_asm_lens_kernel      a thread per contig: length, selected flag, class sums, longest and shortest -- wave
//                          reductions, then one atomic a wave and figure that is not zero.
//  kc_link_tile_scan_kernel / kc_scan_kernel<1>  the two-level scan of the flags.
//  kc_asm_compact_kernel   a thread per contig: a selected one files its index at its rank in block order, and beside it
//                          the sort key longest - length.
//  kc_sort_hist_kernel / kc_sort_scatter_kernel (kc_sort.hpp)  the stable radix passes over the key's significant bits
//                          only: those of longest - shortest.  Equal lengths keep block order.
//  kc_asm_sorted_kernel    a thread per sorted rank: the length again, and the contig of that rank.
//  kc_link_tile_scan_kernel / kc_scan_kernel<1>  the two-level scan of the sorted lengths.
//  kc_asm_nx_kernel        a thread per sorted rank: the rank at which 100 S >= x T first holds is Lx, for x = 50 and 90.
//  kc_asm_spans_kernel     a thread per 4096 bytes: the item (contig of the block; record of the text) that holds the
//                          span's first byte, by a binary search of the 64-bit starts.
//  kc_asm_comp_kernel      the composition, balanced by bytes: a thread per ALIGNED 16 bytes of the block.  The span
//                          table bounds the contigs of a workgroup's bytes (two loads every thread of it shares), a thread
//                          finds the contig of its first byte between them and steps on at every separator.  Sixteen
//                          bytes of one contig that is not selected cost nothing but that; sums per workgroup, then one
//                          atomic a figure, a workgroup taking sixteen spans in turn before that.  Sixteen bases of one
//                          selected contig are counted four words at a time.
// Kernels of kc_fasta_text:
//  kc_asm_text_check_kernel  a thread per offset and per order entry: the offsets contig by contig, the lowest entry of
//                          order that names no contig.
//  kc_asm_sizes_kernel     a thread per record: its bytes.
//  kc_link_tile_scan_kernel / kc_scan_kernel<1>, kc_asm_starts_kernel  the records' 64-bit starts and the total.
//  kc_asm_spans_kernel     as above, over the window.
//  kc_asm_write_kernel     the hot path, output-centric: a thread per ALIGNED 16 bytes of `text`.  The span table bounds
//                          a workgroup's records, a thread finds its record by a search of the starts.  A chunk inside
//                          one line of bases is two aligned 16-byte loads of the block and a funnel shift
//                          (shuf_load16, kc_shuffle.hpp); a chunk of one record's bases with exactly one newline in it is
//                          two of those, a byte mask and the newline; headers, record boundaries, the window's ends and
//                          chunks whose aligned loads would leave the block go byte by byte from (record, position).
//                          Whole chunks leave as one 16-byte store.  A lane divides by the line width once; the id's
//                          digits come from divisions by ten.
//
// No workgroup waits for another; every loop's trip count comes from the input (a search's steps, the records a chunk
// spans, an id's digits).  All figures are integers, so the result does not depend on the order in which the atomics
// arrive.
#pragma once
#include "kc_shuffle.hpp"

namespace kc {

constexpr int ASM_TPB = 256;
constexpr int ASM_SPAN_SHIFT = 12;  // the bytes a workgroup of the byte kernels takes: 256 threads of 16
static_assert((ASM_TPB * 16) == (1 << ASM_SPAN_SHIFT), "a span of the table is a workgroup's bytes");
constexpr int ASM_COMP_SPANS = 16;  // spans a workgroup of the composition takes, one after the other, before its atomics
constexpr int ASM_NCLASSES = 5;
#define ASM_CLASS_LIST {1000u, 5000u, 10000u, 25000u, 50000u}
constexpr int ASM_MAX_PREFIX = 32;

// the status words of kc_ctg_select (AS_SHORTEST starts as all ones) and of kc_fasta_text (AT_BAD_ORDER too)
enum { AS_SELECTED = 0, AS_SEL_BASES, AS_GE_COUNT, AS_GE_BASES = AS_GE_COUNT + ASM_NCLASSES, AS_LONGEST = AS_GE_BASES + ASM_NCLASSES, AS_SHORTEST,
       AS_A, AS_C, AS_G, AS_T, AS_N, AS_N_RUNS, AS_N50, AS_L50, AS_N90, AS_L90, AS_SCAN_SEL, AS_SCAN_BASES, AS_SORT_TOTAL, AS_COUNT };
enum { AT_BAD_OFFSETS = 0, AT_BAD_ORDER, AT_TOTAL, AT_COUNT };

struct AsmSelArgs {
  const uint32_t *offs;  // the n_ctgs + 1 starts in 32 bits (kc_align_check_kernel)
  uint32_t n_ctgs, min_len;
  uint64_t *st;
  uint64_t *flag;        // [n_ctgs] 1 where selected, then the ranks within the tile; later the sorted lengths, likewise
  uint64_t *fbase;       // [tiles] the tiles' bases of either
  uint32_t *sel;         // [n_ctgs] the selected contigs in block order
  uint64_t *keys;        // the compact kernel's output; the sorted keys from then on
  const uint32_t *perm;  // sorted rank -> rank in block order; null: the identity (no pass ran)
  uint64_t nsel;
  uint32_t *by_len;      // [n_ctgs] the selected contigs by length
};

struct AsmRange {
  uint32_t hi, lo;
  __device__ __forceinline__ AsmRange join(const AsmRange &y) const { return AsmRange{y.hi > hi ? y.hi : hi, y.lo < lo ? y.lo : lo}; }
  __device__ __forceinline__ AsmRange across(int o) const { return AsmRange{__shfl_xor(hi, o), __shfl_xor(lo, o)}; }
};

__global__ void __launch_bounds__(ASM_TPB) kc_asm_lens_kernel(AsmSelArgs a) {
  const uint32_t u = blockIdx.x * ASM_TPB + threadIdx.x;
  const bool in = u < a.n_ctgs;
  const uint32_t len = in ? a.offs[u + 1] - 1u - a.offs[u] : 0u;
  const bool sel = in && len >= a.min_len;
  if (in) a.flag[u] = sel ? 1ull : 0ull;
  const bool first = (threadIdx.x & 63) == 0;
  const uint32_t nsel = wave_count(sel);
  if (!nsel) return;  // the whole wave: nothing of it counts
  const uint64_t bases = wave_sum<uint64_t>(sel ? len : 0u);
  // the longest and the shortest in one butterfly (wave_max and wave_min one after the other take two registers more)
  const AsmRange r = wave_join(AsmRange{sel ? len : 0u, sel ? len : 0xFFFFFFFFu});
  const uint32_t hi = r.hi, lo = r.lo;
  if (first) {
    atomicAdd((unsigned long long *)&a.st[AS_SELECTED], (unsigned long long)nsel);
    if (bases) atomicAdd((unsigned long long *)&a.st[AS_SEL_BASES], (unsigned long long)bases);
    if (hi) atomicMax((unsigned long long *)&a.st[AS_LONGEST], (unsigned long long)hi);
    atomicMin((unsigned long long *)&a.st[AS_SHORTEST], (unsigned long long)lo);
  }
  const uint32_t cls[ASM_NCLASSES] = ASM_CLASS_LIST;
#pragma unroll
  for (int j = 0; j < ASM_NCLASSES; j++) {
    const bool ge = sel && len >= cls[j];
    const uint32_t n = wave_count(ge);
    if (!n) break;  // the classes are nested: none of the next either
    const uint64_t s = wave_sum<uint64_t>(ge ? len : 0u);
    if (first) {
      atomicAdd((unsigned long long *)&a.st[AS_GE_COUNT + j], (unsigned long long)n);
      atomicAdd((unsigned long long *)&a.st[AS_GE_BASES + j], (unsigned long long)s);
    }
  }
}

// a.flag, a.fbase: scanned; a.st[AS_LONGEST] is final
__global__ void __launch_bounds__(ASM_TPB) kc_asm_compact_kernel(AsmSelArgs a) {
  const uint32_t u = blockIdx.x * ASM_TPB + threadIdx.x;
  if (u >= a.n_ctgs) return;
  const uint32_t len = a.offs[u + 1] - 1u - a.offs[u];
  if (len < a.min_len) return;
  const uint64_t r = a.fbase[u >> LINK_SCAN_SHIFT] + a.flag[u];
  a.sel[r] = u;
  a.keys[r] = a.st[AS_LONGEST] - len;
}

// a.keys, a.perm: the sorted keys and where they came from
__global__ void __launch_bounds__(ASM_TPB) kc_asm_sorted_kernel(AsmSelArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * ASM_TPB + threadIdx.x;
  if (r >= a.nsel) return;
  a.flag[r] = a.st[AS_LONGEST] - a.keys[r];
  a.by_len[r] = a.sel[a.perm ? a.perm[r] : (uint32_t)r];
}

// a.flag, a.fbase: the sorted lengths, scanned; a.st[AS_SCAN_BASES] their sum T.  With S the sum through rank r and E the
// sum before it, rank r is Lx - 1 iff 100 S >= x T and not 100 E >= x T (r == 0: nothing is before it).
__global__ void __launch_bounds__(ASM_TPB) kc_asm_nx_kernel(AsmSelArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * ASM_TPB + threadIdx.x;
  if (r >= a.nsel) return;
  const uint64_t len = a.st[AS_LONGEST] - a.keys[r], total = a.st[AS_SCAN_BASES];
  const uint64_t e = a.fbase[r >> LINK_SCAN_SHIFT] + a.flag[r], s = e + len;
  if (100 * s >= 50 * total && (r == 0 || 100 * e < 50 * total)) {
    a.st[AS_N50] = len;
    a.st[AS_L50] = r + 1;
  }
  if (100 * s >= 90 * total && (r == 0 || 100 * e < 90 * total)) {
    a.st[AS_N90] = len;
    a.st[AS_L90] = r + 1;
  }
}

// tab[w] = the item of starts[0, n) that holds byte base + 4096 w: n >= 1, starts[0] <= base, the starts increase strictly
__global__ void __launch_bounds__(ASM_TPB) kc_asm_spans_kernel(const uint64_t *starts, uint64_t n, uint64_t base, uint64_t nspans, uint32_t *tab) {
  const uint64_t w = (uint64_t)blockIdx.x * ASM_TPB + threadIdx.x;
  if (w < nspans) tab[w] = (uint32_t)find_le(starts, (uint64_t)0, n - 1, base + (w << ASM_SPAN_SHIFT));
}

// 0x80 in every byte of w that equals ch
__device__ __forceinline__ uint32_t asm_eq_bytes(uint32_t w, uint32_t ch) {
  const uint32_t t = w ^ (ch * 0x01010101u);
  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
}

// Thread t owns seqs[16 t - mis, 16 t - mis + 16) cut to [0, nbytes): mis = seqs' address & 15, so a whole chunk is one
// aligned 16-byte load.  The block is checked (kc_align_check_kernel): n_ctgs >= 1, nbytes >= 1, a separator ends every
// contig, offs[n_ctgs] = nbytes.  A byte counts where its contig is selected.  A workgroup takes ASM_COMP_SPANS consecutive spans
// and adds its sums once: the atomics go to six addresses that all workgroups share, and one span a workgroup leaves the kernel
// bound by them, not by the bytes.
__global__ void __launch_bounds__(ASM_TPB) kc_asm_comp_kernel(const uint8_t *seqs, uint64_t nbytes, const uint64_t *offs, uint64_t n_ctgs,
                                                              uint32_t min_len, const uint32_t *tab, uint64_t *st) {
  const int tid = threadIdx.x;
  const uint64_t mis = (uint64_t)((uintptr_t)seqs & 15u);
  uint32_t cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // A C G T N, runs of N
  for (int s = 0; s < ASM_COMP_SPANS; s++) {  // the spans behind the block's end find no thread with bytes
    const uint64_t t0 = ((uint64_t)blockIdx.x * ASM_COMP_SPANS + s) * ASM_TPB;
    const int64_t p0 = (int64_t)((t0 + tid) * 16) - (int64_t)mis;
    if (p0 < (int64_t)nbytes) {
      // the contigs of the workgroup's first and last byte lie between those of the table's spans around them
      const uint64_t wg_first = t0 * 16 > mis ? t0 * 16 - mis : 0, wg_end = (t0 + ASM_TPB) * 16 - mis;
      const uint64_t w1 = (((wg_end < nbytes ? wg_end : nbytes) - 1) >> ASM_SPAN_SHIFT) + 1;
      const uint64_t lo = tab[wg_first >> ASM_SPAN_SHIFT];
      const uint64_t hi = (w1 << ASM_SPAN_SHIFT) < nbytes ? (uint64_t)tab[w1] : n_ctgs - 1;
      const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < nbytes ? (uint64_t)(p0 + 16) : nbytes;
      uint64_t u = find_le(offs, lo, hi, from);
      uint64_t sep = offs[u + 1] - 1;  // the contig's separator
      bool sel = sep - offs[u] >= min_len;
      if (sel || to > sep) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (to - from == 16) {
          const uint4 x = *(const uint4 *)(seqs + p0);
          w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
        } else {
#pragma unroll
          for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            if (p >= (int64_t)from && p < (int64_t)to) w[j >> 2] |= (uint32_t)seqs[p] << (8 * (j & 3));
          }
        }
        uint32_t prev = from ? seqs[from - 1] : (uint32_t)'_';
        if (sel && to - from == 16 && to <= sep) {  // sixteen bases of one selected contig: four words, no byte on its own
          uint32_t before = prev == 'N' ? 0x80000000u : 0u;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint32_t n = asm_eq_bytes(w[j], 'N');
            cnt[0] += __popc(asm_eq_bytes(w[j], 'A'));
            cnt[1] += __popc(asm_eq_bytes(w[j], 'C'));
            cnt[2] += __popc(asm_eq_bytes(w[j], 'G'));
            cnt[3] += __popc(asm_eq_bytes(w[j], 'T'));
            cnt[4] += __popc(n);
            cnt[5] += __popc(n & ~((n << 8) | (before >> 24)));  // an N whose byte in front is none
            before = n;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            if (p >= (int64_t)from && p < (int64_t)to) {
              const uint32_t ch = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
              if ((uint64_t)p == sep) {  // on to the next contig, if there is one
                u++;
                sel = false;
                if (u < n_ctgs) {
                  const uint64_t nxt = offs[u + 1] - 1;
                  sel = nxt - (sep + 1) >= min_len;
                  sep = nxt;
                }
              } else if (sel) {
                cnt[0] += ch == 'A';
                cnt[1] += ch == 'C';
                cnt[2] += ch == 'G';
                cnt[3] += ch == 'T';
                cnt[4] += ch == 'N';
                cnt[5] += ch == 'N' && prev != 'N';
              }
              prev = ch;
            }
          }
        }
      }
    }
  }
  const int k[6] = {AS_A, AS_C, AS_G, AS_T, AS_N, AS_N_RUNS};
  wg_stats<6>(st, k, cnt);
}

// ---- the text --------------------------------------------------------------------------------------------------------
struct AsmTextArgs {
  const uint8_t *seqs;
  uint64_t nbytes;
  const uint64_t *offs;   // the n_ctgs + 1 starts
  uint64_t n_ctgs;
  const uint32_t *order;  // null: the identity
  uint64_t n_order;
  uint64_t *rs;           // [n_order + 1] the records' bytes, then their starts; the last is the total
  uint64_t *rbase;        // [tiles]
  const uint32_t *tab;    // the record that holds byte first_byte + 4096 w
  const uint8_t *prefix;  // prefix_len bytes in device memory
  uint32_t prefix_len;
  uint32_t lw, lwp1;      // the line's bases, and its bytes; width 0 (one line): 0xFFFFFFFE and 0xFFFFFFFF
  uint64_t first_byte, written;
  uint8_t *text;
  uint64_t *st;
};

// Every offset is compared with nbytes before the byte in front of it is read.
__global__ void __launch_bounds__(ASM_TPB) kc_asm_text_check_kernel(AsmTextArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * ASM_TPB + threadIdx.x;
  if (t <= a.n_ctgs) {
    const uint64_t o = a.offs[t];
    bool ok = o <= a.nbytes;
    if (t == 0) ok &= o == 0;
    if (t == a.n_ctgs) {
      ok &= o == a.nbytes;
    } else {
      const uint64_t nxt = a.offs[t + 1];
      ok &= nxt > o && nxt <= a.nbytes;
      if (ok) ok = a.seqs[nxt - 1] == '_';
    }
    if (!ok) a.st[AT_BAD_OFFSETS] = 1;
  }
  if (a.order && t < a.n_order && a.order[t] >= a.n_ctgs) atomicMin((unsigned long long *)&a.st[AT_BAD_ORDER], (unsigned long long)t);
}

// the offsets and the order are valid from here on
__global__ void __launch_bounds__(ASM_TPB) kc_asm_sizes_kernel(AsmTextArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * ASM_TPB + threadIdx.x;
  if (j >= a.n_order) return;
  const uint32_t u = a.order ? a.order[j] : (uint32_t)j;
  const uint64_t len = a.offs[u + 1] - 1 - a.offs[u];
  const uint64_t lines = a.lwp1 != 0xFFFFFFFFu && len ? (len + a.lw - 1) / a.lw : 1;
  a.rs[j] = 2 + a.prefix_len + dec_digits<10>(u) + len + lines;
}

// a.rs, a.rbase: scanned; a.st[AT_TOTAL] the total
__global__ void __launch_bounds__(ASM_TPB) kc_asm_starts_kernel(AsmTextArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * ASM_TPB + threadIdx.x;
  if (j > a.n_order) return;
  a.rs[j] = j < a.n_order ? a.rbase[j >> LINK_SCAN_SHIFT] + a.rs[j] : a.st[AT_TOTAL];
}

struct AsmRec {
  uint64_t start, end, src;  // the record's bytes in the text; the contig's first byte in the block
  uint32_t u, len, hdr;      // hdr: '>' prefix id '\n'
};

__device__ __forceinline__ AsmRec asm_rec(const AsmTextArgs &a, uint64_t j) {
  AsmRec r;
  r.u = a.order ? a.order[j] : (uint32_t)j;
  r.src = a.offs[r.u];
  r.len = (uint32_t)(a.offs[r.u + 1] - 1 - r.src);
  r.start = a.rs[j];
  r.end = a.rs[j + 1];
  r.hdr = 2u + a.prefix_len + dec_digits<10>(r.u);
  return r;
}

// Thread t owns text[16 t - mis, 16 t - mis + 16) cut to [0, written): mis = text's address & 15, so every whole chunk is
// an aligned 16-byte store.  Byte x of `text` is byte first_byte + x of the whole.  n_order >= 1 and written >= 1.
__global__ void __launch_bounds__(ASM_TPB) kc_asm_write_kernel(AsmTextArgs a) {
  const int tid = threadIdx.x;
  uint8_t *dst = a.text;
  const uint64_t mis = (uint64_t)((uintptr_t)dst & 15u);
  const uint64_t t0 = (uint64_t)blockIdx.x * ASM_TPB;
  if (t0 * 16 >= a.written + mis) return;
  // the records of the workgroup's first and last byte lie between those of the table's spans around them
  const uint64_t wg_first = t0 * 16 > mis ? t0 * 16 - mis : 0, wg_end = (t0 + ASM_TPB) * 16 - mis;
  const uint64_t w1 = (((wg_end < a.written ? wg_end : a.written) - 1) >> ASM_SPAN_SHIFT) + 1;
  const uint64_t lo = a.tab[wg_first >> ASM_SPAN_SHIFT];
  const uint64_t hi = (w1 << ASM_SPAN_SHIFT) < a.written ? (uint64_t)a.tab[w1] : a.n_order - 1;
  const int64_t p0 = (int64_t)((t0 + tid) * 16) - (int64_t)mis;
  if (p0 >= (int64_t)a.written) return;
  const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < a.written ? (uint64_t)(p0 + 16) : a.written;
  uint64_t j = find_le(a.rs, lo, hi, a.first_byte + from);
  AsmRec r = asm_rec(a, j);
  const uint64_t q0 = a.first_byte + from - r.start;  // the first byte's place in its record
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const bool whole = to - from == 16;
  const uintptr_t src_lo = (uintptr_t)a.seqs, src_hi = src_lo + a.nbytes;
  uint32_t col = 0, i = 0;  // in the bases: the place in the line, the base
  bool done = false;
  if (q0 >= r.hdr) {
    const uint32_t b = (uint32_t)(q0 - r.hdr), line = b / a.lwp1;
    col = b - line * a.lwp1;  // col == lw: on the line's newline, i the next line's first base
    i = line * a.lw + col;
    const uintptr_t sa = src_lo + r.src + i;
    const uint64_t cut = (uint64_t)a.lw - col;  // bytes up to the newline
    if (whole && cut >= 16 && (uint64_t)i + 16 <= r.len)
      done = shuf_load16(src_lo, src_hi, sa, w);
    else if (whole && cut < 16 && 15 - cut <= a.lw && (uint64_t)i + 15 <= r.len) {
      // one newline: `cut` bases, the newline, 15 - cut bases of the next line, which come out of sixteen bytes loaded
      // from one byte further to the front
      uint32_t v[4];
      done = shuf_load16(src_lo, src_hi, sa, w) && shuf_load16(src_lo, src_hi, sa - 1, v);
      if (done) {
        const uint32_t c = (uint32_t)cut;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t nb = c > 4u * k ? c - 4u * k : 0u;  // bytes of word k in front of the newline
          const uint32_t m = nb >= 4u ? 0xFFFFFFFFu : (1u << (8u * nb)) - 1u;
          w[k] = (w[k] & m) | (v[k] & ~m);
          if ((c >> 2) == (uint32_t)k) w[k] = (w[k] & ~(0xFFu << (8u * (c & 3u)))) | ((uint32_t)'\n' << (8u * (c & 3u)));
        }
      }
    }
  }
  if (!done) {  // a header, a record's end, an end of the window, lines under sixteen bases, loads that would leave the block
    w[0] = w[1] = w[2] = w[3] = 0u;
    uint64_t bcd = dec_bcd(r.u);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int64_t p = p0 + k;
      uint32_t ch = 0;
      if (p >= (int64_t)from && p < (int64_t)to) {
        const uint64_t g = a.first_byte + (uint64_t)p;
        while (g >= r.end) {  // ends: rs[n_order] = the total > g
          j++;
          r = asm_rec(a, j);
          bcd = dec_bcd(r.u);
        }
        const uint64_t q = g - r.start;
        if (q < r.hdr) {
          ch = q == 0 ? (uint32_t)'>'
             : q <= a.prefix_len ? (uint32_t)a.prefix[q - 1]
             : q + 1 < r.hdr ? (uint32_t)'0' + (uint32_t)((bcd >> (4u * (uint32_t)(r.hdr - 2u - q))) & 15u)
                             : (uint32_t)'\n';
          col = 0;
          i = 0;
        } else if (g + 1 == r.end || col == a.lw) {
          ch = (uint32_t)'\n';
          col = 0;
        } else {
          ch = a.seqs[r.src + i];
          i++;
          col++;
        }
      }
      w[k >> 2] |= ch << (8 * (k & 3));
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
