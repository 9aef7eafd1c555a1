// kc_fastq.hpp -- FASTQ text on the device (kc_fastq_to_packed_device, kc_fastq_pairs_device): the device twins of the
// host parsers kc_fastq_to_packed and kc_fastq_pairs in kc_api.hip, which are their specification byte for byte.
//
// Rules (those of fq_next, kc_api.hip):
//  * Lines end at '\n'; a last line may lack it.  Trailing '\r', ' ' and '\t' are not part of a line.
//  * Record r holds lines 4r .. 4r + 3.  When line 4r is the text's last line and empty, the text ends there.  Else a
//    text with fewer than 4r + 4 lines ends inside record r (a structural error), and so are a name line that is empty
//    or does not start with '@', a third line that is empty or does not start with '+', and sequence and quality lines
//    of different lengths -- checked in that order.  A structurally sound record then has its bases checked against
//    kc_fastq_to_packed's table (mg_code, kc_merge.hpp); the first byte it marks 255 is the error.
//  * Positions are 64-bit throughout: a text may be longer than 2^32 bytes.
//
// Kernels (each file of a pair runs the per-file ones on its own):
//  kc_fq_count_kernel   a workgroup per FQ_TILE bytes: its '\n' count, 16 bytes per lane, compared as words.  Tiles
//                       are laid out from the 16-byte boundary at or below the text's start (FqFile::head), so every
//                       lane's 16 bytes are one aligned load wherever the text starts; only the chunks holding the
//                       text's first or last byte are read a byte at a time.
//  kc_scan_kernel<1>    (kc_scan.hpp) one workgroup: exclusive scan of a u64 array in place, and its total.  It turns
//                       the tile counts into each tile's first line number, and the per-workgroup sequence sums into
//                       output offsets.
//  kc_fq_index_kernel   a workgroup per tile again: every '\n' gets its line number and stores its position, so line L
//                       ends at ends[L] (8 bytes per line, 32 per record).
//  kc_fq_check_kernel   a lane per record: the structural checks, the sequence length; then its wave walks the bases of
//                       its 64 records, 64 at a time, against the table.  The smallest failing record of each kind goes
//                       to an atomicMin key.
//  kc_fq_detail_kernel  one wave: what the host needs to rebuild the host parser's message for the winning keys.
//  kc_fq_sums_kernel    sequence lengths summed per FQ_TPB records in output order (file 1, file 2, file 1, ... when
//                       two files are interleaved).
//  kc_fq_write_kernel   per FQ_TPB output records: in-workgroup offsets on the scanned sums, then a wave per record
//                       writes the bytes (<packed>: code | min(q - qual_offset, 31) << 3 with the host's wrap-around;
//                       <pairs>: bases and qualities as they are) and the read offsets, for the records the host would
//                       have written before it stopped, while they fit the arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_common.hpp"
#include "kc_kit.hpp"
#include "kc_merge.hpp"

namespace kc {

constexpr int FQ_TPB = 256;
constexpr int FQ_VEC = 16;    // text bytes per lane and step
constexpr int FQ_STEPS = 16;  // steps per tile
constexpr uint64_t FQ_TILE = (uint64_t)FQ_TPB * FQ_VEC * FQ_STEPS;  // 64 KiB
constexpr unsigned FQ_MAX_GRID = 1u << 20;  // grid-stride loops beyond this many workgroups
constexpr uint64_t FQ_NONE = ~0ull;

// per-file control words (u64): set to FQ_NONE before the kernels run
enum { FQC_STRUCT = 0, FQC_BASE, FQC_END, FQC_KIND, FQC_A, FQC_B, FQC_POS, FQC_BYTE, FQC_CONSUMED, FQC_NNL, FQC_TOTAL, FQC_N = 16 };
// FQC_KIND of a structural error
enum { FQK_TRUNCATED = 1, FQK_NAME, FQK_PLUS, FQK_LENGTH };

struct FqFile {
  const uint8_t *text;
  uint64_t len;
  uint64_t head;   // text's offset above the 16-byte boundary below it: the tiles cover [text - head, text + len)
  uint64_t *tile;  // [ntiles] '\n' counts, then (kc_scan_kernel) each tile's first line number
  uint64_t ntiles;
  uint64_t *ends;  // [nnl] position of each '\n'
  uint64_t nnl;    // '\n' bytes in the text
  uint64_t nl;     // lines parsed: nnl, one more for a last line without '\n', 4 * whole records under KC_FASTQ_PARTIAL
  uint64_t nrec;   // candidate records, ceil(nl / 4)
  uint64_t *slen;  // [nrec] sequence length of a sound record, else 0
  uint64_t *ctl;   // [FQC_N]
};

struct FqOut {
  uint8_t *packed;     // <packed>
  uint8_t *bases;      // <pairs>
  uint8_t *quals;
  uint64_t *offsets;   // [reads_cap + 1]
  uint64_t cap;        // output bytes
  uint64_t reads_cap;
  uint64_t nout;       // output records in the sums' order (what kc_fq_sums_kernel covered)
  uint64_t lim;        // records [0, lim) are written where they fit
  uint64_t part_rec;   // FQ_NONE, or the record whose bases [0, part_len) are written (a bad base in <packed>)
  uint64_t part_len;
  uint64_t *bsum;      // scanned per-workgroup sums
  int qoff;
};

// line i ends here: ends[i], or the text's end for a last line without '\n'
__device__ __forceinline__ uint64_t fq_end(const FqFile &f, uint64_t i) { return i < f.nnl ? f.ends[i] : f.len; }

__device__ __forceinline__ bool fq_ws(uint32_t c) { return c == '\r' || c == ' ' || c == '\t'; }

// [b, e) without its trailing white space
__device__ __forceinline__ uint64_t fq_strip(const uint8_t *t, uint64_t b, uint64_t e) {
  while (e > b && fq_ws(t[e - 1])) e--;
  return e;
}

// zero-byte mask of a word: bit 7 of each byte that equals '\n' (exact, no carries between bytes)
__device__ __forceinline__ uint32_t fq_nl_nibble(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
  return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// bit j set: byte P + j of the aligned view is a '\n' of the text.  P counts from the 16-byte boundary at or below the
// text's start (a multiple of 16); bytes below f.head or at or past f.head + f.len are not the text's and are not read.
__device__ __forceinline__ uint32_t fq_nl_mask(const FqFile &f, uint64_t P) {
  const uint8_t *t = f.text - f.head;  // 16-byte aligned
  const uint64_t lo = f.head, hi = f.head + f.len;
  uint32_t w[4];
  if (P >= lo && P + 16 <= hi) {
    const uint4 v = *(const uint4 *)(t + P);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
  } else {
    for (int k = 0; k < 4; k++) {
      uint32_t x = 0;
      for (int j = 0; j < 4; j++) {
        const uint64_t q = P + 4 * k + j;
        x |= (uint32_t)(q >= lo && q < hi ? t[q] : 0u) << (8 * j);
      }
      w[k] = x;
    }
  }
  return fq_nl_nibble(w[0]) | fq_nl_nibble(w[1]) << 4 | fq_nl_nibble(w[2]) << 8 | fq_nl_nibble(w[3]) << 12;
}

__global__ void __launch_bounds__(FQ_TPB) kc_fq_count_kernel(FqFile f) {
  __shared__ uint32_t wsum[FQ_TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint64_t tile = blockIdx.x; tile < f.ntiles; tile += gridDim.x) {
    const uint64_t t0 = tile * FQ_TILE + (uint64_t)tid * FQ_VEC;
    uint32_t n = 0;
    for (int s = 0; s < FQ_STEPS; s++) n += __popc(fq_nl_mask(f, t0 + (uint64_t)s * FQ_TPB * FQ_VEC));
    n = wave_sum(n);
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (tid == 0) {
      uint64_t t = 0;
      for (int w = 0; w < FQ_TPB / 64; w++) t += wsum[w];
      f.tile[tile] = t;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(FQ_TPB) kc_fq_index_kernel(FqFile f) {
  __shared__ uint32_t wsum[FQ_TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint64_t tile = blockIdx.x; tile < f.ntiles; tile += gridDim.x) {
    uint64_t line = f.tile[tile];
    for (int s = 0; s < FQ_STEPS; s++) {
      const uint64_t p = tile * FQ_TILE + (uint64_t)s * FQ_TPB * FQ_VEC + (uint64_t)tid * FQ_VEC;
      uint32_t m = fq_nl_mask(f, p);
      const uint32_t c = __popc(m);
      uint32_t inc = c;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
      }
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      uint32_t pre = inc - c, tot = 0;
      for (int w = 0; w < FQ_TPB / 64; w++) {
        const uint32_t x = wsum[w];
        if (w < wv) pre += x;
        tot += x;
      }
      uint64_t idx = line + pre;
      while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1;
        if (idx < f.nnl) f.ends[idx] = p + j - f.head;  // a '\n' is never below head
        idx++;
      }
      line += tot;
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(FQ_TPB) kc_fq_check_kernel(FqFile f) {
  const int tid = threadIdx.x, lane = tid & 63;
  const uint8_t *t = f.text;
  for (uint64_t blk = blockIdx.x; blk * FQ_TPB < f.nrec; blk += gridDim.x) {
    const uint64_t r = blk * FQ_TPB + tid;
    int ok = 0;
    uint64_t sb = 0, sl = 0;
    if (r < f.nrec) {
      const uint64_t L = 4 * r;
      const uint64_t b0 = L ? fq_end(f, L - 1) + 1 : 0, e0 = fq_end(f, L), e0s = fq_strip(t, b0, e0);
      if (L + 1 == f.nl && e0s == b0) {
        f.ctl[FQC_END] = 1;  // a final empty line
      } else if (L + 3 >= f.nl) {
        atomicMin((unsigned long long *)&f.ctl[FQC_STRUCT], (unsigned long long)r);
      } else {
        const uint64_t e1 = fq_end(f, L + 1), e2 = fq_end(f, L + 2), e3 = fq_end(f, L + 3);
        const uint64_t b1 = e0 + 1, b2 = e1 + 1, b3 = e2 + 1;
        const uint64_t e1s = fq_strip(t, b1, e1), e2s = fq_strip(t, b2, e2), e3s = fq_strip(t, b3, e3);
        if (e0s == b0 || t[b0] != '@' || e2s == b2 || t[b2] != '+' || e1s - b1 != e3s - b3) {
          atomicMin((unsigned long long *)&f.ctl[FQC_STRUCT], (unsigned long long)r);
        } else {
          ok = 1;
          sb = b1;
          sl = e1s - b1;
        }
      }
      f.slen[r] = ok ? sl : 0;
    }
    // the wave walks its 64 records' bases
    const uint64_t r0 = r - lane;
    for (int j = 0; j < 64; j++) {
      if (!__shfl(ok, j)) continue;
      const uint64_t sbj = __shfl(sb, j), slj = __shfl(sl, j);
      for (uint64_t i0 = 0; i0 < slj; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool bad = i < slj && mg_code(t[sbj + i]) == 255u;
        if (__ballot(bad)) {
          if (lane == 0) atomicMin((unsigned long long *)&f.ctl[FQC_BASE], (unsigned long long)(r0 + j));
          break;
        }
      }
    }
  }
}

// one wave: the details of the winning keys, and where the parsed text ends
__global__ void __launch_bounds__(64) kc_fq_detail_kernel(FqFile f) {
  const int lane = threadIdx.x;
  const uint8_t *t = f.text;
  if (lane == 0) f.ctl[FQC_CONSUMED] = f.nl ? min(fq_end(f, f.nl - 1) + 1, f.len) : 0;
  const uint64_t rs = f.ctl[FQC_STRUCT];
  if (rs != FQ_NONE && lane == 0) {
    const uint64_t L = 4 * rs;
    uint64_t kind = FQK_TRUNCATED, a = 0, b = 0;
    if (L + 3 < f.nl) {
      const uint64_t b0 = L ? fq_end(f, L - 1) + 1 : 0, e0 = fq_end(f, L);
      const uint64_t e1 = fq_end(f, L + 1), e2 = fq_end(f, L + 2), e3 = fq_end(f, L + 3);
      const uint64_t b1 = e0 + 1, b2 = e1 + 1, b3 = e2 + 1;
      const uint64_t e0s = fq_strip(t, b0, e0), e1s = fq_strip(t, b1, e1), e2s = fq_strip(t, b2, e2), e3s = fq_strip(t, b3, e3);
      if (e0s == b0 || t[b0] != '@') kind = FQK_NAME;
      else if (e2s == b2 || t[b2] != '+') kind = FQK_PLUS;
      else kind = FQK_LENGTH;
      a = e1s - b1;
      b = e3s - b3;
    }
    f.ctl[FQC_KIND] = kind;
    f.ctl[FQC_A] = a;
    f.ctl[FQC_B] = b;
  }
  const uint64_t rb = f.ctl[FQC_BASE];
  if (rb != FQ_NONE) {
    const uint64_t L = 4 * rb, b1 = fq_end(f, L) + 1, sl = f.slen[rb];
    for (uint64_t i0 = 0; i0 < sl; i0 += 64) {
      const uint64_t i = i0 + lane;
      const bool bad = i < sl && mg_code(t[b1 + i]) == 255u;
      const unsigned long long m = __ballot(bad);
      if (m) {
        const int j = __ffsll(m) - 1;
        if (lane == j) {
          f.ctl[FQC_POS] = i;
          f.ctl[FQC_BYTE] = t[b1 + i];
        }
        break;
      }
    }
  }
}

// sequence length of output record g: file 1's record g, or with two files file (g & 1)'s record g / 2
__device__ __forceinline__ uint64_t fq_len_at(const FqFile &f0, const FqFile &f1, int two, uint64_t g) {
  const bool second = two && (g & 1);
  const uint64_t r = two ? g >> 1 : g;
  const uint64_t nrec = second ? f1.nrec : f0.nrec;
  const uint64_t *slen = second ? f1.slen : f0.slen;
  return r < nrec ? slen[r] : 0;
}

__global__ void __launch_bounds__(FQ_TPB) kc_fq_sums_kernel(FqFile f0, FqFile f1, int two, uint64_t nout, uint64_t *bsum) {
  __shared__ uint64_t wsum[FQ_TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint64_t blk = blockIdx.x; blk * FQ_TPB < nout; blk += gridDim.x) {
    const uint64_t g = blk * FQ_TPB + tid;
    uint64_t v = g < nout ? fq_len_at(f0, f1, two, g) : 0;
    v = wave_sum(v);
    if (lane == 0) wsum[wv] = v;
    __syncthreads();
    if (tid == 0) {
      uint64_t s = 0;
      for (int w = 0; w < FQ_TPB / 64; w++) s += wsum[w];
      bsum[blk] = s;
    }
    __syncthreads();
  }
}

template <bool PACKED>
__global__ void __launch_bounds__(FQ_TPB) kc_fq_write_kernel(FqFile f0, FqFile f1, int two, FqOut o) {
  __shared__ uint64_t wsum[FQ_TPB / 64];
  __shared__ uint64_t s_off[FQ_TPB], s_len[FQ_TPB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t nw = o.part_rec != FQ_NONE ? o.part_rec + 1 : o.lim;  // part_rec >= lim
  for (uint64_t blk = blockIdx.x; blk * FQ_TPB < nw; blk += gridDim.x) {
    const uint64_t g = blk * FQ_TPB + tid;
    const uint64_t sl = g < o.nout ? fq_len_at(f0, f1, two, g) : 0;
    uint64_t inc = sl;
    for (int k = 1; k < 64; k <<= 1) {
      const uint64_t x = __shfl_up(inc, k);
      if (lane >= k) inc += x;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint64_t off = o.bsum[blk] + inc - sl;
    for (int w = 0; w < wv; w++) off += wsum[w];
    const bool fits = g < o.reads_cap && off + sl <= o.cap;
    uint64_t wl = 0;
    if (fits && g < o.lim) {
      o.offsets[g + 1] = off + sl;
      wl = sl;
    } else if (fits && g == o.part_rec) {
      wl = o.part_len;
    }
    s_off[tid] = off;
    s_len[tid] = wl;
    __syncthreads();
    for (int j = wv; j < FQ_TPB; j += FQ_TPB / 64) {
      const uint64_t n = s_len[j];
      if (!n) continue;
      const uint64_t gj = blk * FQ_TPB + j;
      const bool second = two && (gj & 1);  // the fields picked one by one: a picked struct would go to scratch
      const uint8_t *text = second ? f1.text : f0.text;
      const uint64_t *ends = second ? f1.ends : f0.ends;
      const uint64_t nnl = second ? f1.nnl : f0.nnl, len = second ? f1.len : f0.len;
      const uint64_t r = two ? gj >> 1 : gj, L = 4 * r;
      const uint64_t sb = (L < nnl ? ends[L] : len) + 1, qb = (L + 2 < nnl ? ends[L + 2] : len) + 1, dst = s_off[j];
      for (uint64_t i = lane; i < n; i += 64) {
        const uint32_t b = text[sb + i], q = text[qb + i];
        if (PACKED) {
          int qq = (int)q - o.qoff;
          if (qq > 31) qq = 31;
          o.packed[dst + i] = (uint8_t)(mg_code(b) | ((uint32_t)(uint8_t)qq << 3));
        } else {
          o.bases[dst + i] = (uint8_t)b;
          o.quals[dst + i] = (uint8_t)q;
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace kc
