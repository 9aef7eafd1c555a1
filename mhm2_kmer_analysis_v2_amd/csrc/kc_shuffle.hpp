// kc_shuffle.hpp -- the read pairs regrouped by their home contig (kc_shuffle_reads): the role of
// shuffle_reads(qual_offset, packed_reads_list, ctgs), src/contigging.cpp:128-147, commented out in the proxy.  The
// reference holds no code for it (no shuffle_reads in src/), so the rules are this project's own definition (DESIGN.md
// section 22, pinned statement by statement by tests/shuffle_model.py); no parity with MetaHipMer is claimed.
// include/kcount_mi355.h states the rules in full.
//
// Kernels, in the order of the call (the checks in front of them are kc_align_lengths_kernel, kc_depth_check_kernel and
// kc_lassm_pair_check_kernel):
//  kc_shuf_longest_kernel  a thread per contig: the longest contig (wave maximum, one atomicMax a wave); its bit length is
//                          the width of the key's anchor field.
//  kc_shuf_key_kernel      a thread per pair: the two candidates, the chosen record, the key home << abits | anchor (a
//                          homeless pair: n_ctgs << abits), and the pairs' classes summed per workgroup before any atomic.
//  kc_sort_hist_kernel / kc_sort_scatter_kernel (kc_sort.hpp)  the stable radix passes over the key's significant bits
//                          only: abits + the bits of n_ctgs.  Equal keys keep the old pair order.
//  kc_shuf_place_kernel    a thread per sorted rank: the new pair index by the parts rule, order, home, the inverse
//                          permutation, the two mates' lengths in new order (one 16-byte store) and the pair's old byte
//                          offset; a thread at the end of a home's run finds the run's start by a binary search of the
//                          sorted keys: the distinct homes and the largest home (wave sums and maxima, then one atomic).
//  kc_link_tile_scan_kernel / kc_scan_kernel<1>  the two-level scan of the lengths.
//  kc_shuf_offsets_kernel  a thread per new offset: tile base + in-tile sum; the last is the total.  The thread of a pair's
//                          first read also files the pair under the 4096-byte block of the output whose first byte it
//                          holds (a pair has at most 2048 bytes: at most one), so that the gather starts its search there.
//  kc_shuf_gather_kernel   the hot path, output-centric: a thread per ALIGNED 16 bytes of the output block, bases
//                          (blockIdx.y 0) and qualities (1) in one launch.  The block table bounds the pairs of a
//                          workgroup's bytes (two loads every thread of it shares), every thread then finds its own pair
//                          between them by a search of the new offsets: a few steps.  A chunk inside one pair
//                          is two aligned 16-byte loads of the source and a funnel shift by the source's misalignment; a
//                          chunk over the boundary of two pairs is two of those, one from either pair's source, and a
//                          byte mask; a chunk over three pairs or more, at an end of the block, or whose aligned loads
//                          would leave the source array goes byte by byte.  Whole chunks leave as one 16-byte store.
//  kc_shuf_remap_kernel    a thread per record (read = 2 * inverse[read / 2] + read % 2, two 16-byte loads and stores)
//                          and, behind the records, a thread per new pair (pairs_out[q] = pairs[order[q]]).
//  kc_shuf_parts_kernel    a thread per part boundary.
//
// No workgroup waits for another; every loop's trip count comes from the input (a search's steps, the pairs a chunk
// spans).  All figures are integers, so the result does not depend on the order in which the atomics arrive.
#pragma once
#include "kc_links.hpp"
#include "kc_sort.hpp"

namespace kc {

constexpr int SHUF_TPB = 256;
constexpr uint32_t SHUF_NO_ALN = 0xFFFFFFFFu, SHUF_NO_HOME = 0xFFFFFFFFu;
constexpr uint32_t SHUF_MAX_PARTS = 65536;
constexpr int SHUF_BLOCK_SHIFT = 12;  // the bytes a workgroup of the gather writes: 256 threads of 16
static_assert((SHUF_TPB * 16) == (1 << SHUF_BLOCK_SHIFT), "a block of the table is a workgroup's bytes");
static_assert(2 * ALIGN_MAX_READ_LEN < (1 << SHUF_BLOCK_SHIFT), "a pair holds the first byte of at most one block");

enum { SHS_HOMED = 0, SHS_ONE_MATE, SHS_TWO_SAME, SHS_TWO_DIFF, SHS_HOMES, SHS_MAX_HOME, SHS_LONGEST, SHS_BYTES, SHS_SORT_TOTAL, SHS_COUNT };

struct ShufArgs {
  const uint32_t *offs;  // the index's n_ctgs + 1 starts
  uint32_t n_ctgs, abits, parts;
  const uint4 *alns;  // kc_gap_aln
  uint64_t n_alns;
  const uint4 *pairs;  // kc_pair_rec
  uint64_t npairs;
  const uint64_t *offsets;  // the reads'
  uint64_t *st;
  uint64_t *keys;        // [npairs] the key kernel's output; the sorted keys for the place kernel
  const uint32_t *perm;  // [npairs] sorted rank -> old pair; null: the identity (no pass ran)
  uint64_t *lens;        // [nreads] the reads' lengths in new order, then their sums within their tile
  uint64_t *lbase;       // [tiles of reads] the tiles' first bytes
  uint64_t *psrc;        // [npairs] a new pair's old byte offset
  uint32_t *blk;         // [ceil(bytes / 4096)] the new pair that holds byte 4096 w
  uint32_t *inv;         // [npairs] old pair -> new pair
  uint32_t *order, *home;
  uint64_t *offsets_out, *part_starts;
  uint4 *alns_out, *pairs_out;  // either may be null
};

// what the gather reads: stream 0 the bases, stream 1 the qualities (absent: one stream is launched)
struct ShufCopy {
  const uint8_t *src[2];
  uint8_t *dst[2];
  const uint64_t *noff;  // the nreads + 1 new offsets
  const uint64_t *psrc;
  const uint32_t *blk;
  uint64_t npairs, total;
};

__global__ void __launch_bounds__(SHUF_TPB) kc_shuf_longest_kernel(const uint32_t *offs, uint32_t n_ctgs, uint64_t *st) {
  const uint32_t u = blockIdx.x * SHUF_TPB + threadIdx.x;
  const uint32_t len = wave_max(u < n_ctgs ? offs[u + 1] - 1u - offs[u] : 0u);
  if ((threadIdx.x & 63) == 0 && len) atomicMax((unsigned long long *)&st[SHS_LONGEST], (unsigned long long)len);
}

// the records are valid (kc_depth_check_kernel) and the pairs are (kc_lassm_pair_check_kernel)
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_shuf_key_kernel(ShufArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int cls = -1;
  if (p < a.npairs) {
    const uint4 pr = a.pairs[p];
    const bool has0 = pr.x != SHUF_NO_ALN, has1 = pr.y != SHUF_NO_ALN;
    uint64_t key = (uint64_t)a.n_ctgs << a.abits;
    if (has0 || has1) {
      const DepthRec r0 = depth_load(a.alns, has0 ? pr.x : pr.y), r1 = depth_load(a.alns, has1 ? pr.y : pr.x);
      // mate 1's record is chosen only where it comes strictly first
      const bool second = has0 && has1 &&
                          (r1.score > r0.score ||
                           (r1.score == r0.score && (r1.ctg < r0.ctg || (r1.ctg == r0.ctg && r1.cstart < r0.cstart))));
      const uint32_t ctg = second ? r1.ctg : r0.ctg, cstart = second ? r1.cstart : r0.cstart;
      key = ((uint64_t)ctg << a.abits) | cstart;
      cls = !(has0 && has1) ? SHS_ONE_MATE : r0.ctg == r1.ctg ? SHS_TWO_SAME : SHS_TWO_DIFF;
    }
    a.keys[p] = key;
  }
  const int k[4] = {SHS_HOMED, SHS_ONE_MATE, SHS_TWO_SAME, SHS_TWO_DIFF};
  const uint32_t mine[4] = {cls >= 0 ? 1u : 0u, cls == SHS_ONE_MATE ? 1u : 0u, cls == SHS_TWO_SAME ? 1u : 0u, cls == SHS_TWO_DIFF ? 1u : 0u};
  wg_stats<4>(a.st, k, mine);
}

// the part of rank r of a segment of n pairs dealt over `parts`: floor(((r + 1) * parts - 1) / n), below 2^47
__device__ __forceinline__ uint64_t shuf_part(uint64_t r, uint64_t n, uint64_t parts) { return ((r + 1) * parts - 1) / n; }

// a.keys, a.perm: the sorted keys and where they came from; a.st[SHS_HOMED] is final
__global__ void __launch_bounds__(SHUF_TPB) kc_shuf_place_kernel(ShufArgs a) {
  __shared__ uint32_t heads[SHUF_TPB / 64], longest[SHUF_TPB / 64];
  const int tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.x * SHUF_TPB + tid;
  const uint64_t nh = a.st[SHS_HOMED], nu = a.npairs - nh, parts = a.parts;
  bool head = false;
  uint32_t run = 0;
  if (r < a.npairs) {
    const uint64_t key = a.keys[r], p = a.perm ? (uint64_t)a.perm[r] : r;
    const uint32_t h = (uint32_t)(key >> a.abits);
    uint64_t q;
    if (r < nh) {
      q = r + shuf_part(r, nh, parts) * nu / parts;
      head = r == 0 || (uint32_t)(a.keys[r - 1] >> a.abits) != h;
      if (r + 1 == nh || (uint32_t)(a.keys[r + 1] >> a.abits) != h) {  // the last of its home: where does the home begin
        const uint64_t want = (uint64_t)h << a.abits;
        uint64_t lo = 0, hi = r;
        while (lo < hi) {
          const uint64_t mid = lo + ((hi - lo) >> 1);
          if (a.keys[mid] < want)
            lo = mid + 1;
          else
            hi = mid;
        }
        run = (uint32_t)(r - lo) + 1u;
      }
    } else {
      const uint64_t u = r - nh;
      q = u + (shuf_part(u, nu, parts) + 1) * nh / parts;
    }
    const uint64_t o0 = a.offsets[2 * p], o1 = a.offsets[2 * p + 1], o2 = a.offsets[2 * p + 2];
    a.order[q] = (uint32_t)p;
    a.home[q] = r < nh ? h : SHUF_NO_HOME;
    a.inv[p] = (uint32_t)q;
    a.psrc[q] = o0;
    ulonglong2 l;
    l.x = o1 - o0;
    l.y = o2 - o1;
    *(ulonglong2 *)(a.lens + 2 * q) = l;
  }
  const uint32_t nheads = wave_count(head);
  run = wave_max(run);
  if ((tid & 63) == 0) {
    heads[tid >> 6] = nheads;
    longest[tid >> 6] = run;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t n = 0, m = 0;
    for (int w = 0; w < SHUF_TPB / 64; w++) {
      n += heads[w];
      m = longest[w] > m ? longest[w] : m;
    }
    if (n) atomicAdd((unsigned long long *)&a.st[SHS_HOMES], (unsigned long long)n);
    if (m) atomicMax((unsigned long long *)&a.st[SHS_MAX_HOME], (unsigned long long)m);
  }
}

// a.lens, a.lbase: scanned; a.st[SHS_BYTES] the total
__global__ void __launch_bounds__(SHUF_TPB) kc_shuf_offsets_kernel(ShufArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * SHUF_TPB + threadIdx.x, nreads = 2 * a.npairs;
  if (i > nreads) return;
  const uint64_t total = a.st[SHS_BYTES];
  const uint64_t s = i < nreads ? a.lbase[i >> LINK_SCAN_SHIFT] + a.lens[i] : total;
  a.offsets_out[i] = s;
  if (i < nreads && !(i & 1)) {  // a pair's first read: the pair is [s, e)
    const uint64_t e = i + 2 < nreads ? a.lbase[(i + 2) >> LINK_SCAN_SHIFT] + a.lens[i + 2] : total;
    const uint64_t w = (s + ((1ull << SHUF_BLOCK_SHIFT) - 1)) >> SHUF_BLOCK_SHIFT;
    if ((w << SHUF_BLOCK_SHIFT) < e) a.blk[w] = (uint32_t)(i >> 1);
  }
}

// The sixteen bytes at address sa as four dwords: two aligned 16-byte loads (one where sa is aligned) and a funnel shift by
// sa's misalignment -- the dword part by selects on constant indices, the byte part by v_alignbyte.  False, and nothing
// loaded, where an aligned load would leave [lo, hi).
__device__ __forceinline__ bool shuf_load16(uintptr_t lo, uintptr_t hi, uintptr_t sa, uint32_t (&w)[4]) {
  const uintptr_t sh = sa & 15u, at = sa - sh;
  if (at < lo || at + (sh ? 32u : 16u) > hi) return false;
  const uint4 x = *(const uint4 *)at, y = sh ? *(const uint4 *)(at + 16) : x;
  const uint32_t ws = (uint32_t)sh >> 2, bs = (uint32_t)sh & 3u;
  const uint32_t v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
  uint32_t m[5];
#pragma unroll
  for (int j = 0; j < 5; j++) m[j] = ws == 0 ? v[j] : ws == 1 ? v[j + 1] : ws == 2 ? v[j + 2] : v[j + 3];
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = __builtin_amdgcn_alignbyte(m[j + 1], m[j], bs);
  return true;
}

// Thread t of a stream owns out[16 t - mis, 16 t - mis + 16) cut to [0, total): mis = out's address & 15, so every whole
// chunk is an aligned 16-byte store.  npairs >= 1 and total >= 1 (the host launches nothing otherwise).
__global__ void __launch_bounds__(SHUF_TPB) kc_shuf_gather_kernel(ShufCopy a) {
  const int tid = threadIdx.x, s = blockIdx.y;
  const uint8_t *src = a.src[s];
  uint8_t *dst = a.dst[s];
  const uint64_t mis = (uint64_t)((uintptr_t)dst & 15u);
  const uint64_t t0 = (uint64_t)blockIdx.x * SHUF_TPB;
  if (t0 * 16 >= a.total + mis) return;  // the whole workgroup: the streams' misalignments differ
  // the pairs of the workgroup's first and last byte lie between those of the table's blocks around them
  const uint64_t first = t0 * 16 > mis ? t0 * 16 - mis : 0, end = (t0 + SHUF_TPB) * 16 - mis;  // end: at least 4096 - 15
  const uint64_t w1 = (((end < a.total ? end : a.total) - 1) >> SHUF_BLOCK_SHIFT) + 1;
  const uint64_t lo = a.blk[first >> SHUF_BLOCK_SHIFT];
  const uint64_t hi = (w1 << SHUF_BLOCK_SHIFT) < a.total ? (uint64_t)a.blk[w1] : a.npairs - 1;
  const int64_t p0 = (int64_t)((t0 + tid) * 16) - (int64_t)mis;
  if (p0 >= (int64_t)a.total) return;
  const uint64_t from = p0 < 0 ? 0ull : (uint64_t)p0, to = (uint64_t)(p0 + 16) < a.total ? (uint64_t)(p0 + 16) : a.total;
  // the greatest q whose pair starts at or before `from` (noff[0] = 0)
  const uint64_t *noff = a.noff;
  uint64_t q = find_le(lo, hi, from, [noff](uint64_t mid) { return noff[2 * mid]; });
  uint64_t pstart = a.noff[2 * q], pend = a.noff[2 * q + 2], sp = a.psrc[q];
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const bool whole = to - from == 16;
  const uintptr_t src_lo = (uintptr_t)src, src_hi = src_lo + a.total, sa = src_lo + sp + (from - pstart);
  bool done = false;
  if (whole && to <= pend)
    done = shuf_load16(src_lo, src_hi, sa, w);
  else if (whole && q + 1 < a.npairs && to <= a.noff[2 * q + 4]) {
    // two pairs: `cut` bytes (1 .. 15: the search gave a pair that holds `from`) end pair q, the others begin pair q + 1;
    // either comes out of sixteen bytes loaded from where the chunk would lie in that pair's source
    const uint32_t cut = (uint32_t)(pend - from);
    uint32_t v[4];
    done = shuf_load16(src_lo, src_hi, sa, w) && shuf_load16(src_lo, src_hi, src_lo + a.psrc[q + 1] - cut, v);
    if (done) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t nb = cut > 4u * j ? cut - 4u * j : 0u;  // bytes of word j that are pair q's
        const uint32_t m = nb >= 4u ? 0xFFFFFFFFu : (1u << (8u * nb)) - 1u;
        w[j] = (w[j] & m) | (v[j] & ~m);
      }
    }
  }
  if (!done) {  // an end of the block, a chunk over three pairs or more, or aligned loads that would leave the source array
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      uint32_t c = 0;
      if (p >= (int64_t)from && p < (int64_t)to) {
        while ((uint64_t)p >= pend) {  // ends: noff[2 * npairs] = total > p
          q++;
          pstart = pend;
          pend = a.noff[2 * q + 2];
          sp = a.psrc[q];
        }
        c = src[sp + ((uint64_t)p - pstart)];
      }
      w[j >> 2] |= c << (8 * (j & 3));
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
}

__global__ void __launch_bounds__(SHUF_TPB) kc_shuf_remap_kernel(ShufArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * SHUF_TPB + threadIdx.x;
  const uint64_t nrec = a.alns_out ? a.n_alns : 0;
  if (i < nrec) {
    uint4 x = a.alns[2 * i];
    const uint4 y = a.alns[2 * i + 1];
    x.x = 2u * a.inv[x.x >> 1] + (x.x & 1u);
    a.alns_out[2 * i] = x;
    a.alns_out[2 * i + 1] = y;
  } else if (a.pairs_out && i - nrec < a.npairs) {
    const uint64_t q = i - nrec;
    a.pairs_out[q] = a.pairs[a.order[q]];
  }
}

__global__ void __launch_bounds__(SHUF_TPB) kc_shuf_parts_kernel(ShufArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * SHUF_TPB + threadIdx.x, parts = a.parts;
  if (j > parts) return;
  const uint64_t nh = a.st[SHS_HOMED], nu = a.npairs - nh;
  a.part_starts[j] = j * nh / parts + j * nu / parts;
}

}  // namespace kc
