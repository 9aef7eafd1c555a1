// kc_fasta_in.hpp -- FASTA text to a seq block on the device (kc_fasta_to_block): the inverse of kc_fasta_text (kc_asm.hpp),
// the contig side's twin of the FASTQ parser (kc_fastq.hpp).  The reference holds no Contigs::load_contigs, so the rules are
// this project's own definition (pinned statement by statement by tests/fasta_in_model.py); no parity
// with MetaHipMer is claimed.  include/kcount_mi355.h states the rules in full.
//
// The line index is the FASTQ parser's as it stands: kc_fq_count_kernel, kc_scan_kernel<1> and kc_fq_index_kernel leave
// every '\n' position in ends[].  Behind it, in the order of the call:
//  kc_fa_lines_kernel   a thread per line: the stripped extent; a header (first byte '>') counts 1, the separator in front
//                       of its record, a sequence line its bytes; the flags "header" and "non-empty sequence line"; under
//                       KC_FASTA_PARTIAL the last header line, by one atomicMax a wave.
//  kc_link_tile_scan_kernel / kc_scan_kernel<1>  three two-level scans over the lines: V (block bytes in front of a line,
//                       plus one), H (headers in front of it) and E (non-empty sequence lines in front of it).
//  kc_fa_starts_kernel  a thread per line: the scans' tile bases are added in place; a header line files its line under
//                       its record and gives the record's offset V.
//  kc_fa_spans_kernel   a thread per 4096 bytes: the line that holds the span's first byte -- of the text, by the lines'
//                       starts, or of the block, by V.
//  kc_fa_check_kernel   the validation, balanced by bytes: a thread per ALIGNED 16 bytes of the text.  The span table bounds
//                       a workgroup's lines, a thread finds the line of its first byte between them.  Sixteen bytes inside
//                       one sequence line are one load, tested through the two bit masks of mg_code (kc_merge.hpp) with no
//                       branch a byte; a chunk that crosses a line end goes byte by byte.  The smallest bad position goes to
//                       a 64-bit atomicMin (2 * position + kind, so that a sequence line in front of the first header wins
//                       over a bad base at its first byte), the records' LOWERED / RECODED flags to an atomicOr that a
//                       plain load in front of it spares wherever the flag already stands.
//  kc_fa_detail_kernel  one thread: line, column and byte of the winning position.
//  kc_fa_recs_kernel    a thread per record: the header parse (at most KC_FASTA_HDR_SCAN bytes) and kc_fasta_rec.
//  kc_fa_write_kernel   the hot path, output-centric: a thread per ALIGNED 16 bytes of the block.  The span table bounds a
//                       workgroup's lines, a thread finds its line by a search of V.  A chunk inside one line is two aligned
//                       16-byte loads of the text and a funnel shift (shuf_load16, kc_shuffle.hpp), recoded four bytes a
//                       word; a chunk over a line end or a separator goes byte by byte.  Whole chunks leave as one 16-byte
//                       store, and their depths as the matching 32 bytes.
//
// Block byte x and the lines: with y = x + 1, the line i with V[i] <= y < V[i + 1] holds it -- a sequence line its base
// y - V[i], a header line the separator of the record in front of it, the line behind the last (V[nl] = the block's bytes)
// the last record's separator.  The first header's own count is byte -1, which nobody asks for.
//
// No workgroup waits for another; every loop's trip count comes from the input (a search's steps, a line's trailing
// blanks, the lines a chunk spans, a header's first 256 bytes).  All figures are integers, so the result does not depend on
// the order in which the atomics arrive.
#pragma once
#include "kc_asm.hpp"
#include "kc_fastq.hpp"

namespace kc {

constexpr int FA_TPB = 256;
constexpr int FA_SPAN_SHIFT = 12;  // the bytes a workgroup of the byte kernels takes: 256 threads of 16
static_assert((FA_TPB * 16) == (1 << FA_SPAN_SHIFT), "a span of the table is a workgroup's bytes");
constexpr uint32_t FA_HDR_SCAN = 256;
constexpr uint32_t FA_HAS_ID = 1u, FA_HAS_DEPTH = 2u, FA_LOWERED = 4u, FA_RECODED = 8u;
constexpr uint64_t FA_STRICT_BITS = mg_bits("ACGTN");

// the status words: FAS_KEY starts as all ones, the others as zero
enum { FAS_KEY = 0, FAS_LAST, FAS_NNL, FAS_NBYTES, FAS_HEADERS, FAS_SEQ_LINES, FAS_LOWERED, FAS_RECODED, FAS_EMPTY_RECS, FAS_LONGEST, FAS_WITH_ID,
       FAS_WITH_DEPTH, FAS_ERR_LINE, FAS_ERR_COL, FAS_ERR_BYTE, FAS_COUNT };

struct FaRec {  // kc_fasta_rec
  uint64_t hdr_pos;
  uint32_t hdr_len, seq_lines;
  uint64_t id;
  uint32_t depth, flags;
};
static_assert(sizeof(FaRec) == 32, "the header's record");

struct FaArgs {
  const uint8_t *text;
  uint64_t len;          // under KC_FASTA_PARTIAL: the bytes in front of the last header
  const uint64_t *ends;  // [nnl] the position of every '\n'
  uint64_t nnl, nl;      // '\n' bytes in text[0, len), and lines: one more for a last line without '\n'
  uint64_t *v, *h, *e;   // [nl + 1] per line, see above: counts, then scanned within tiles, then (kc_fa_starts_kernel) final
  uint64_t *vbase, *hbase, *ebase;  // [tiles]
  uint64_t *st;
  uint64_t n_ctgs, nbytes;
  uint64_t *hline;       // [n_ctgs + 1] the header line of a record; the last is nl
  uint64_t *roff;        // [n_ctgs + 1] the block's offsets
  uint32_t *rflags;      // [n_ctgs] FA_LOWERED, FA_RECODED
  FaRec *recs;           // [n_ctgs]
  const uint64_t *tab;   // the line that holds byte 4096 w of the text (check) or of the block (write)
  uint32_t strict, default_depth;
  uint8_t *seqs;
  uint16_t *depths;      // may be null
};

__device__ __forceinline__ uint64_t fa_begin(const FaArgs &a, uint64_t i) { return i ? a.ends[i - 1] + 1 : 0; }
__device__ __forceinline__ uint64_t fa_end(const FaArgs &a, uint64_t i) { return i < a.nnl ? a.ends[i] : a.len; }

// a.len, a.nnl, a.nl: those of the whole text
__global__ void __launch_bounds__(FA_TPB) kc_fa_lines_kernel(FaArgs a, int partial) {
  const uint64_t i = (uint64_t)blockIdx.x * FA_TPB + threadIdx.x;
  uint64_t last = 0;
  if (i < a.nl) {
    const uint64_t b = fa_begin(a, i), e = fa_end(a, i);
    const bool hdr = e > b && a.text[b] == '>';
    const uint64_t n = hdr ? 0 : fq_strip(a.text, b, e) - b;
    a.v[i] = hdr ? 1 : n;
    a.h[i] = hdr ? 1 : 0;
    a.e[i] = n ? 1 : 0;
    last = hdr ? i + 1 : 0;
  }
  if (partial) {
    last = wave_max(last);
    if ((threadIdx.x & 63) == 0 && last) atomicMax((unsigned long long *)&a.st[FAS_LAST], (unsigned long long)last);
  }
}

// the three arrays are scanned within their tiles; a.n_ctgs, a.nbytes and st[FAS_SEQ_LINES] are the totals
__global__ void __launch_bounds__(FA_TPB) kc_fa_starts_kernel(FaArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * FA_TPB + threadIdx.x;
  if (i > a.nl) return;
  const bool in = i < a.nl;
  const uint64_t t = i >> LINK_SCAN_SHIFT;
  const uint64_t v = in ? a.vbase[t] + a.v[i] : a.nbytes, h = in ? a.hbase[t] + a.h[i] : a.n_ctgs, e = in ? a.ebase[t] + a.e[i] : a.st[FAS_SEQ_LINES];
  a.v[i] = v;
  a.h[i] = h;
  a.e[i] = e;
  bool hdr = !in;  // the line behind the last ends the last record
  if (in) {
    const uint64_t b = fa_begin(a, i);
    hdr = fa_end(a, i) > b && a.text[b] == '>';
  }
  if (hdr) {
    a.hline[h] = i;
    a.roff[h] = v;
  }
}

// the greatest i in [lo, hi] whose line starts at or before byte x of the text (lo's does)
__device__ __forceinline__ uint64_t fa_line_of(const FaArgs &a, uint64_t lo, uint64_t hi, uint64_t x) {
  const uint64_t *ends = a.ends;
  return find_le(lo, hi, x, [ends](uint64_t mid) { return ends[mid - 1] + 1; });  // mid > lo >= 0
}

// by_block 0: tab[w] = the line that holds byte 4096 w of the text (nl >= 1); 1: the line i of [0, nl] with
// V[i] <= 4096 w + 1 < V[i + 1]
__global__ void __launch_bounds__(FA_TPB) kc_fa_spans_kernel(FaArgs a, int by_block, uint64_t nspans, uint64_t *tab) {
  const uint64_t w = (uint64_t)blockIdx.x * FA_TPB + threadIdx.x;
  if (w >= nspans) return;
  const uint64_t x = w << FA_SPAN_SHIFT;
  tab[w] = by_block ? find_le(a.v, (uint64_t)0, a.nl, x + 1) : fa_line_of(a, 0, a.nl - 1, x);
}

// a line as the check walks it
struct FaLine {
  uint64_t b, send, nlp, rec;  // first byte; end of the sequence bytes (b: none); the '\n' or the text's end; headers in front of it
};

__device__ __forceinline__ FaLine fa_line(const FaArgs &a, uint64_t i) {
  FaLine l;
  l.b = fa_begin(a, i);
  l.nlp = fa_end(a, i);
  const bool hdr = l.nlp > l.b && a.text[l.b] == '>';
  l.send = hdr ? l.b : l.b + (a.v[i + 1] - a.v[i]);
  l.rec = a.h[i];
  return l;
}

__device__ __forceinline__ bool fa_ok(uint32_t c, uint64_t acc) { return (c >> 6) == 1u && ((acc >> (c & 63u)) & 1u); }

__device__ __forceinline__ void fa_flag(const FaArgs &a, uint64_t rec, uint32_t f) {
  if (!f || !rec) return;
  uint32_t *p = a.rflags + (rec - 1);
  if ((*(volatile uint32_t *)p & f) != f) atomicOr(p, f);
}

// Thread t owns text[16 t - head, 16 t - head + 16) cut to [0, len): head = text's address & 15, so a whole chunk is one
// aligned 16-byte load.  len >= 1 and nl >= 1; the arrays per line and hline are final.
__global__ void __launch_bounds__(FA_TPB) kc_fa_check_kernel(FaArgs a) {
  const int tid = threadIdx.x;
  const uint8_t *text = a.text;
  const uint64_t head = (uint64_t)((uintptr_t)text & 15u);
  const uint64_t t0 = (uint64_t)blockIdx.x * FA_TPB;
  const uint64_t acc = a.strict ? FA_STRICT_BITS : (MG_ACGT | MG_FOUR);
  const uint64_t first = a.n_ctgs ? a.hline[0] : a.nl;  // the lines in front of it are in front of the first header
  uint32_t cnt[2] = {0u, 0u};                            // lowered, recoded
  uint64_t key = FQ_NONE;
  const int64_t p0 = (int64_t)((t0 + tid) * 16) - (int64_t)head;
  if (t0 * 16 < a.len + head && p0 < (int64_t)a.len) {
    // the lines of the workgroup's first and last byte lie between those of the table's spans around them
    const uint64_t wg_first = t0 * 16 > head ? t0 * 16 - head : 0, wg_end = (t0 + FA_TPB) * 16 - head;
    const uint64_t w1 = (((wg_end < a.len ? wg_end : a.len) - 1) >> FA_SPAN_SHIFT) + 1;
    const uint64_t lo = a.tab[wg_first >> FA_SPAN_SHIFT];
    const uint64_t hi = (w1 << FA_SPAN_SHIFT) < a.len ? a.tab[w1] : a.nl - 1;
    const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < a.len ? (uint64_t)(p0 + 16) : a.len;
    uint64_t i = fa_line_of(a, lo, hi, from);
    FaLine l = fa_line(a, i);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const bool whole = to - from == 16;
    if (whole) {
      const uint4 x = *(const uint4 *)(text + p0);
      w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int64_t p = p0 + j;
        if (p >= (int64_t)from && p < (int64_t)to) w[j >> 2] |= (uint32_t)text[p] << (8 * (j & 3));
      }
    }
    bool done = false;
    if (whole && to <= l.send) {  // sixteen bytes of one sequence line: no byte on its own unless one is bad
      bool ok = true;
      uint32_t low = 0, plain = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int k = 0; k < 4; k++) ok &= fa_ok((w[j] >> (8 * k)) & 0xFFu, acc);
        const uint32_t up = w[j] & 0xDFDFDFDFu;
        low += __popc(w[j] & 0x20202020u);
        plain += __popc(asm_eq_bytes(up, 'A') | asm_eq_bytes(up, 'C') | asm_eq_bytes(up, 'G') | asm_eq_bytes(up, 'T') | asm_eq_bytes(up, 'N'));
      }
      if (ok) {
        done = true;
        cnt[0] += low;
        cnt[1] += 16u - plain;
        fa_flag(a, l.rec, (low ? FA_LOWERED : 0u) | (plain != 16u ? FA_RECODED : 0u));
        if (from == l.b && i < first) key = 2 * from;
      }
    }
    if (!done) {
      uint32_t f = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int64_t p = p0 + j;
        if (p >= (int64_t)from && p < (int64_t)to) {
          const uint64_t q = (uint64_t)p;
          if (q > l.nlp) {  // a line has a byte at least, its '\n': one step
            fa_flag(a, l.rec, f);
            f = 0;
            i++;
            l = fa_line(a, i);
          }
          if (q < l.send) {
            const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            uint64_t k = FQ_NONE;
            if (q == l.b && i < first) k = 2 * q;
            else if (!fa_ok(c, acc)) k = 2 * q + 1;
            else {
              const bool lowc = (c & 0x20u) != 0, plainc = ((FA_STRICT_BITS >> (c & 0x1Fu)) & 1u) != 0;  // (of an accepted byte)
              cnt[0] += lowc;
              cnt[1] += !plainc;
              f |= (lowc ? FA_LOWERED : 0u) | (!plainc ? FA_RECODED : 0u);
            }
            key = k < key ? k : key;
          }
        }
      }
      fa_flag(a, l.rec, f);
    }
  }
  key = wave_min(key);
  if ((tid & 63) == 0 && key != FQ_NONE) atomicMin((unsigned long long *)&a.st[FAS_KEY], (unsigned long long)key);
  const int k[2] = {FAS_LOWERED, FAS_RECODED};
  wg_stats<2>(a.st, k, cnt);
}

// one thread: the line, the column and the byte of the winning position
__global__ void __launch_bounds__(64) kc_fa_detail_kernel(FaArgs a) {
  if (threadIdx.x) return;
  const uint64_t key = a.st[FAS_KEY];
  if (key == FQ_NONE) return;
  const uint64_t p = key >> 1, i = fa_line_of(a, 0, a.nl - 1, p);
  a.st[FAS_ERR_LINE] = i + 1;
  a.st[FAS_ERR_COL] = p - fa_begin(a, i) + 1;
  a.st[FAS_ERR_BYTE] = a.text[p];
}

__device__ __forceinline__ bool fa_blank(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool fa_digit(uint32_t c) { return c - (uint32_t)'0' < 10u; }

// a thread per record; rflags is final (kc_fa_check_kernel has run)
__global__ void __launch_bounds__(FA_TPB) kc_fa_recs_kernel(FaArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * FA_TPB + threadIdx.x;
  uint32_t cnt[3] = {0u, 0u, 0u};  // empty records, with id, with depth
  uint64_t len = 0;
  if (r < a.n_ctgs) {
    const uint64_t i = a.hline[r], nxt = a.hline[r + 1];
    const uint8_t *t = a.text + fa_begin(a, i);
    const uint64_t hl = fq_strip(a.text, fa_begin(a, i), fa_end(a, i)) - fa_begin(a, i), lines = a.e[nxt] - a.e[i];
    const uint32_t n = hl < FA_HDR_SCAN ? (uint32_t)hl : FA_HDR_SCAN;
    const bool open = hl > FA_HDR_SCAN;  // a token that reaches byte 256 does not end inside the bytes looked at
    FaRec rec;
    rec.hdr_pos = fa_begin(a, i);
    rec.hdr_len = hl < 0xFFFFFFFFull ? (uint32_t)hl : 0xFFFFFFFFu;
    rec.seq_lines = lines < 0xFFFFFFFFull ? (uint32_t)lines : 0xFFFFFFFFu;
    rec.id = 0;
    rec.depth = a.default_depth;
    rec.flags = a.rflags[r];
    uint32_t t1 = 1;
    while (t1 < n && !fa_blank(t[t1])) t1++;
    if (!(t1 == n && open)) {
      uint32_t nd = 0;
      while (t1 - nd > 1 && fa_digit(t[t1 - nd - 1])) nd++;
      if (nd >= 1 && nd <= 18) {
        uint64_t id = 0;
        for (uint32_t j = t1 - nd; j < t1; j++) id = id * 10 + (t[j] - (uint32_t)'0');
        rec.id = id;
        rec.flags |= FA_HAS_ID;
      }
      uint32_t s2 = t1;
      while (s2 < n && fa_blank(t[s2])) s2++;
      uint32_t t2 = s2;
      while (t2 < n && !fa_blank(t[t2])) t2++;
      if (t2 > s2 && !(t2 == n && open)) {
        uint32_t j = s2, whole = 0, ni = 0;
        while (j < t2 && fa_digit(t[j])) {
          if (ni < 9) whole = whole * 10 + (t[j] - (uint32_t)'0');
          ni++;
          j++;
        }
        bool ok = ni >= 1 && ni <= 9;
        uint32_t up = 0;
        if (ok && j < t2) {
          ok = t[j] == '.';
          j++;
          if (ok && j < t2) up = fa_digit(t[j]) && t[j] >= '5';
          while (ok && j < t2) ok = fa_digit(t[j]), j++;
        }
        if (ok) {
          const uint32_t d = whole + up;
          rec.depth = d < 65535u ? d : 65535u;
          rec.flags |= FA_HAS_DEPTH;
        }
      }
    }
    a.recs[r] = rec;
    len = a.roff[r + 1] - 1 - a.roff[r];
    cnt[0] = len == 0;
    cnt[1] = (rec.flags & FA_HAS_ID) != 0;
    cnt[2] = (rec.flags & FA_HAS_DEPTH) != 0;
  }
  len = wave_max(len);
  if ((threadIdx.x & 63) == 0 && len) atomicMax((unsigned long long *)&a.st[FAS_LONGEST], (unsigned long long)len);
  const int k[3] = {FAS_EMPTY_RECS, FAS_WITH_ID, FAS_WITH_DEPTH};
  wg_stats<3>(a.st, k, cnt);
}

// a line as the writer walks it: block bytes [v0 - 1, v1 - 1) are its
struct FaSrc {
  uint64_t v0, v1, b;
  uint32_t depth;
  bool seq;  // else a separator
};

__device__ __forceinline__ FaSrc fa_src(const FaArgs &a, uint64_t i) {
  FaSrc s;
  s.v0 = a.v[i];
  s.v1 = ~0ull;
  s.b = 0;
  s.depth = 0;
  s.seq = false;
  if (i < a.nl) {
    s.v1 = a.v[i + 1];
    s.b = fa_begin(a, i);
    s.seq = s.v1 > s.v0 && a.text[s.b] != '>';
    if (s.seq && a.depths) s.depth = a.recs[a.h[i] - 1].depth;  // the text is valid: a sequence line has a header in front
  }
  return s;
}

// four accepted bytes as the block holds them: ACGT of either case as upper case, the others 'N'
__device__ __forceinline__ uint32_t fa_recode(uint32_t w) {
  const uint32_t up = w & 0xDFDFDFDFu;
  const uint32_t z = asm_eq_bytes(up, 'A') | asm_eq_bytes(up, 'C') | asm_eq_bytes(up, 'G') | asm_eq_bytes(up, 'T');
  const uint32_t m = (z >> 7) * 0xFFu;
  return (up & m) | (0x4E4E4E4Eu & ~m);
}

// Thread t owns seqs[16 t - mis, 16 t - mis + 16) cut to [0, nbytes): mis = seqs' address & 15, so every whole chunk is an
// aligned 16-byte store.  The text is valid, nbytes >= 1 (hence nl >= 1 and n_ctgs >= 1).
__global__ void __launch_bounds__(FA_TPB) kc_fa_write_kernel(FaArgs a) {
  const int tid = threadIdx.x;
  uint8_t *dst = a.seqs;
  const uint64_t mis = (uint64_t)((uintptr_t)dst & 15u);
  const uint64_t t0 = (uint64_t)blockIdx.x * FA_TPB;
  if (t0 * 16 >= a.nbytes + mis) return;
  const uint64_t wg_first = t0 * 16 > mis ? t0 * 16 - mis : 0, wg_end = (t0 + FA_TPB) * 16 - mis;
  const uint64_t w1 = (((wg_end < a.nbytes ? wg_end : a.nbytes) - 1) >> FA_SPAN_SHIFT) + 1;
  const uint64_t lo = a.tab[wg_first >> FA_SPAN_SHIFT];
  const uint64_t hi = (w1 << FA_SPAN_SHIFT) < a.nbytes ? a.tab[w1] : a.nl;
  const int64_t p0 = (int64_t)((t0 + tid) * 16) - (int64_t)mis;
  if (p0 >= (int64_t)a.nbytes) return;
  const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < a.nbytes ? (uint64_t)(p0 + 16) : a.nbytes;
  uint64_t i = find_le(a.v, lo, hi, from + 1);
  FaSrc s = fa_src(a, i);
  uint32_t w[4] = {0u, 0u, 0u, 0u}, d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const bool whole = to - from == 16;
  const uintptr_t src_lo = (uintptr_t)a.text, src_hi = src_lo + a.len;
  bool done = false;
  if (whole && s.seq && to + 1 <= s.v1) {
    done = shuf_load16(src_lo, src_hi, src_lo + s.b + (from + 1 - s.v0), w);
    if (done) {
#pragma unroll
      for (int j = 0; j < 4; j++) w[j] = fa_recode(w[j]);
#pragma unroll
      for (int j = 0; j < 8; j++) d[j] = s.depth * 0x00010001u;
    }
  }
  if (!done) {  // a line's end, a separator, an end of the block, loads that would leave the text
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      uint32_t ch = 0, dp = 0;
      if (p >= (int64_t)from && p < (int64_t)to) {
        const uint64_t y = (uint64_t)p + 1;
        while (y >= s.v1) {  // ends: the line behind the last has no end
          i++;
          s = fa_src(a, i);
        }
        ch = (uint32_t)'_';
        if (s.seq) {
          ch = fa_recode(a.text[s.b + (y - s.v0)]) & 0xFFu;
          dp = s.depth;
        }
      }
      w[j >> 2] |= ch << (8 * (j & 3));
      d[j >> 1] |= dp << (16 * (j & 1));
    }
  }
  if (whole)
    *(uint4 *)(dst + p0) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      if (p >= (int64_t)from && p < (int64_t)to) dst[p] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
  if (a.depths) {
    if (whole && (((uintptr_t)(a.depths + p0)) & 15u) == 0) {
      *(uint4 *)(a.depths + p0) = make_uint4(d[0], d[1], d[2], d[3]);
      *(uint4 *)(a.depths + p0 + 8) = make_uint4(d[4], d[5], d[6], d[7]);
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int64_t p = p0 + j;
        if (p >= (int64_t)from && p < (int64_t)to) a.depths[p] = (uint16_t)(d[j >> 1] >> (16 * (j & 1)));
      }
    }
  }
}

}  // namespace kc
