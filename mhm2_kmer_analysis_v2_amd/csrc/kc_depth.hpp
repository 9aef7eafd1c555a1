// kc_depth.hpp -- what the gapped records are for: per-base and per-contig depths (kc_aln_depths) and the pairs' classes
// and insert sizes (kc_pair_inserts): the role of histogrammer.calculate_insert_size(alns) behind find_alignments
// (src/contigging.cpp:164) and of the depths the contig pass is fed.  The reference holds no code for either (no Alns, no
// CtgsDepths, no histogrammer in src/), so the rules are this project's own definition (pinned
// statement by statement by tests/depth_model.py); no parity with MetaHipMer is claimed.
//
// Rules (include/kcount_mi355.h states them in full):
//  * A record (kc_gap_aln) is valid iff ctg < n_ctgs, orient <= 1, kind <= 2 and, unless kind is KC_GAP_NONE,
//    cstart < cstop <= len_u and rstart < rstop <= KC_ALIGN_MAX_READ_LEN; where the call uses reads, read < nreads, and
//    where it has their lengths, rstop <= L(read) unless kind is KC_GAP_NONE.
//  * It passes the filter iff kind != KC_GAP_NONE, score >= min_score and cstop - cstart >= min_len.
//  * A read's best record: the greatest score among those that pass, the lowest index among equal scores -- one 64-bit
//    atomicMax of score << 32 | (0xFFFFFFFF - index) into a word per read (0: none; an index is below 2^32 - 1).
//  * A record that passes adds 1 to the contig positions [lo, hi), lo = cstart + (cstart > 0 ? e : 0),
//    hi = cstop - (cstop < len_u ? e : 0), iff lo < hi.
//
// Kernels:
//  kc_depth_check_kernel      a thread per record: validity, the lowest bad index by a 64-bit atomicMin.  Stores nothing else.
//  kc_depth_best_kernel       a thread per record: the atomicMax above.
//  kc_depth_mark_kernel       a thread per record: its class for the statistics, and for a contributing one +1 at
//                             offs[u] + lo and -1 at offs[u] + hi of a 32-bit difference array over the block (modular), and
//                             one more alignment of contig u.  hi <= len_u, so a contig's differences cancel at or before
//                             its separator: one prefix sum over the whole block gives every depth.
//  kc_depth_tile_sums_kernel  the sum of every tile of DEPTH_TILE differences; kc_scan_kernel<1> (kc_scan.hpp) turns the
//                             tile sums into the tiles' bases.
//  kc_depth_rescan_kernel     a tile again: base + the inclusive scan, eight consecutive bytes a thread, written as
//                             saturated 16-bit depths (one 16-byte store a thread) and folded into the per-contig figures
//                             while the thread holds them.
//  kc_depth_ctg_kernel        a thread per contig: mean and the 32-byte record.
//  kc_depth_fill_kernel       KC_DEPTH_PER_CONTIG: every byte gets its contig's mean (the means exist only after the rescan).
//  kc_pair_classify_kernel<LDS>  a thread per pair: the two best words, the two records, the class, the 16-byte record; the
//                             histogram in LDS bins (max_insert < PAIR_LDS_BINS) or by global 64-bit atomics.
//
// Per-contig figures, per byte with segmented wave reductions and integer atomics: a thread walks its eight bytes with
// the contig of the first (a binary search between the tile's first and last contig, which two threads of the workgroup
// find first: no steps at all inside a long contig, a few on cached lines among short ones).  A segment that begins and
// ends inside the thread goes to its contig directly; the segment open at the thread's end is combined across the lanes by
// a segmented scan (a lane that holds a separator starts a segment) and is folded in by the lane that holds the
// contig's separator, or by lane 63.  So a contig gets one set of atomics per wave it spans plus one per separator: a
// megabase contig about 2000 a million bases, a 40-base contig one or two, whatever the mix of lengths is.  A wave
// per contig would leave a megabase contig to one wave, and a thread per contig strides through memory.  sum and covered
// are added, min and max go through atomicMin / atomicMax; an add of 0, a max of 0 and a min of 0xFFFFFFFF are skipped.
// No workgroup waits for another: every loop's trip count comes from the input (the search by n_ctgs, the walk by 8).
#pragma once
#include "kc_gap.hpp"
#include "kc_scan.hpp"

namespace kc {

constexpr int DEPTH_TPB = 256;
constexpr int DEPTH_ITEMS = 8;                            // consecutive bytes a thread holds: one 16-byte store of depths
constexpr uint32_t DEPTH_TILE = DEPTH_TPB * DEPTH_ITEMS;  // 2048 differences a workgroup
constexpr uint32_t DEPTH_MAX_EDGE = 1024;                 // KC_DEPTH_MAX_EDGE
constexpr uint32_t DEPTH_BEST_ONLY = 1, DEPTH_PER_CONTIG = 2;
constexpr uint32_t PAIR_LDS_BINS = 8192;  // 32 KiB of 32-bit bins: two workgroups a compute unit keep theirs
constexpr uint32_t PAIR_INSERT_MAX = 65535;
constexpr int PAIR_TPB = 256;
constexpr uint32_t PAIR_NONE = 0, PAIR_ONE = 1, PAIR_DIFF_CTG = 2, PAIR_SAME_ORIENT = 3, PAIR_EVERTED = 4, PAIR_TOO_LONG = 5, PAIR_PROPER = 6;
constexpr int PAIR_CLASSES = 7;

enum { DPS_BAD = 0, DPS_NONE, DPS_FILTERED, DPS_NOT_BEST, DPS_CLIPPED, DPS_USED, DPS_COVERED, DPS_DEPTH_SUM, DPS_SATURATED, DPS_TOTAL,
       DPS_COUNT };
enum { PRS_CLS = 0, PRS_INSERT_SUM = PAIR_CLASSES, PRS_INSERT_SQ, PRS_WITH_BEST, PRS_COUNT };

struct DepthArgs {
  const uint32_t *offs;  // the index's n_ctgs + 1 starts
  uint32_t n_ctgs, nbytes;
  const uint4 *alns;  // kc_gap_aln, two words of 16 bytes each
  uint64_t n_alns, nreads;
  const uint64_t *offsets;  // the reads' (kc_pair_inserts) or null
  uint32_t min_score, min_len, edge_clip, flags;
  uint64_t *best;       // [nreads] or null
  uint32_t *diff;       // [tiles * DEPTH_TILE]
  uint64_t *tile_sums;  // [tiles]
  uint64_t *csum;       // [n_ctgs] each: the contigs' partial figures
  uint32_t *ccov, *cmin, *cmax, *calns, *cmean;
  uint16_t *depths;  // [nbytes] or null
  uint4 *ctgs;       // kc_ctg_depth[n_ctgs] or null
  uint64_t *st;
};

struct DepthRec {
  uint32_t read, ctg, cstart, cstop, rstart, rstop, score, orient, kind;
};

__device__ __forceinline__ DepthRec depth_load(const uint4 *alns, uint64_t i) {
  const uint4 a = alns[2 * i], z = alns[2 * i + 1];
  DepthRec r;
  r.read = a.x;
  r.ctg = a.y;
  r.cstart = a.z;
  r.cstop = a.w;
  r.rstart = z.x & 0xFFFFu;
  r.rstop = z.x >> 16;
  r.score = z.y;
  r.orient = z.w & 0xFFu;
  r.kind = (z.w >> 8) & 0xFFu;
  return r;
}

__device__ __forceinline__ bool depth_passes(const DepthArgs &a, const DepthRec &r) {
  return r.kind != GAP_KIND_NONE && r.score >= a.min_score && r.cstop - r.cstart >= a.min_len;
}

__device__ __forceinline__ uint64_t depth_best_word(uint32_t score, uint64_t i) { return ((uint64_t)score << 32) | (0xFFFFFFFFull - i); }

// use_reads: read < nreads is part of validity; with a.offsets also rstop <= the read's length
__global__ void kc_depth_check_kernel(DepthArgs a, int use_reads) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_alns) return;
  const DepthRec r = depth_load(a.alns, i);
  bool ok = r.ctg < a.n_ctgs && r.orient <= 1u && r.kind <= GAP_KIND_NONE;
  if (ok && r.kind != GAP_KIND_NONE) {
    const uint32_t len = a.offs[r.ctg + 1] - 1u - a.offs[r.ctg];
    ok = r.cstart < r.cstop && r.cstop <= len && r.rstart < r.rstop && r.rstop <= (uint32_t)ALIGN_MAX_READ_LEN;
  }
  if (use_reads) {
    ok = ok && (uint64_t)r.read < a.nreads;
    if (ok && a.offsets && r.kind != GAP_KIND_NONE) ok = (uint64_t)r.rstop <= a.offsets[r.read + 1] - a.offsets[r.read];
  }
  if (!ok) atomicMin((unsigned long long *)&a.st[DPS_BAD], (unsigned long long)i);
}

__global__ void kc_depth_best_kernel(DepthArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_alns) return;
  const DepthRec r = depth_load(a.alns, i);
  if (depth_passes(a, r)) atomicMax((unsigned long long *)&a.best[r.read], (unsigned long long)depth_best_word(r.score, i));
}

__global__ void kc_depth_mark_kernel(DepthArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int cls = -1;  // DPS_NONE .. DPS_USED
  if (i < a.n_alns) {
    const DepthRec r = depth_load(a.alns, i);
    if (r.kind == GAP_KIND_NONE)
      cls = DPS_NONE;
    else if (!depth_passes(a, r))
      cls = DPS_FILTERED;
    else if ((a.flags & DEPTH_BEST_ONLY) && a.best[r.read] != depth_best_word(r.score, i))
      cls = DPS_NOT_BEST;
    else {
      const uint32_t o = a.offs[r.ctg], len = a.offs[r.ctg + 1] - 1u - o;
      const int64_t lo = (int64_t)r.cstart + (r.cstart > 0u ? (int64_t)a.edge_clip : 0);
      const int64_t hi = (int64_t)r.cstop - (r.cstop < len ? (int64_t)a.edge_clip : 0);
      if (lo >= hi)
        cls = DPS_CLIPPED;
      else {  // 0 <= lo < hi <= len: both inside [offs[u], the separator]
        cls = DPS_USED;
        atomicAdd(&a.diff[o + (uint32_t)lo], 1u);
        atomicAdd(&a.diff[o + (uint32_t)hi], 0xFFFFFFFFu);
        atomicAdd(&a.calns[r.ctg], 1u);
      }
    }
  }
#pragma unroll
  for (int k = DPS_NONE; k <= DPS_USED; k++) {
    const uint32_t n = wave_count(cls == k);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long *)&a.st[k], (unsigned long long)n);
  }
}

// the thread's eight differences as inclusive sums of its own, and their total
__device__ __forceinline__ uint32_t depth_load8(const uint32_t *diff, uint32_t j0, uint32_t (&d)[DEPTH_ITEMS]) {
  const uint4 *p = (const uint4 *)(diff + j0);
  const uint4 x = p[0], y = p[1];
  d[0] = x.x;
  d[1] = d[0] + x.y;
  d[2] = d[1] + x.z;
  d[3] = d[2] + x.w;
  d[4] = d[3] + y.x;
  d[5] = d[4] + y.y;
  d[6] = d[5] + y.z;
  d[7] = d[6] + y.w;
  return d[7];
}

__global__ void __launch_bounds__(DEPTH_TPB) kc_depth_tile_sums_kernel(DepthArgs a) {
  __shared__ uint32_t ws[DEPTH_TPB / 64];
  const int tid = threadIdx.x;
  uint32_t d[DEPTH_ITEMS];
  const uint32_t s = wave_sum(depth_load8(a.diff, blockIdx.x * DEPTH_TILE + (uint32_t)tid * DEPTH_ITEMS, d));
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) a.tile_sums[blockIdx.x] = (uint64_t)(ws[0] + ws[1] + ws[2] + ws[3]);  // modulo 2^32, like every depth
}
static_assert(DEPTH_TPB == 256, "four waves a workgroup");

// the tile's first and last contig into range[0], range[1] (thread 0 and thread 64: two waves); the caller synchronises.
// A byte's contig is the greatest u with offs[u] <= the byte (the starts increase strictly: every contig has its separator).
__device__ __forceinline__ void depth_tile_range(const DepthArgs &a, uint32_t tile0, uint32_t *range) {
  if (threadIdx.x == 0) range[0] = find_le(a.offs, 0u, a.n_ctgs - 1u, tile0);
  if (threadIdx.x == 64) {
    const uint32_t last = tile0 + DEPTH_TILE - 1u;
    range[1] = find_le(a.offs, 0u, a.n_ctgs - 1u, last < a.nbytes ? last : a.nbytes - 1u);
  }
}

struct DepthSeg {
  uint64_t sum;
  uint32_t cov, mn, mx;
  __device__ __forceinline__ DepthSeg join(const DepthSeg &y) const {
    return DepthSeg{sum + y.sum, cov + y.cov, mn < y.mn ? mn : y.mn, mx > y.mx ? mx : y.mx};
  }
  __device__ __forceinline__ DepthSeg up(int o) const { return DepthSeg{__shfl_up(sum, o), __shfl_up(cov, o), __shfl_up(mn, o), __shfl_up(mx, o)}; }
};
__device__ __forceinline__ DepthSeg depth_seg_none() { return DepthSeg{0ull, 0u, 0xFFFFFFFFu, 0u}; }
__device__ __forceinline__ void depth_seg_flush(const DepthArgs &a, uint32_t u, const DepthSeg &s) {
  if (u >= a.n_ctgs) return;
  if (s.sum) atomicAdd((unsigned long long *)&a.csum[u], (unsigned long long)s.sum);
  if (s.cov) atomicAdd(&a.ccov[u], s.cov);
  if (s.mn != 0xFFFFFFFFu) atomicMin(&a.cmin[u], s.mn);
  if (s.mx) atomicMax(&a.cmax[u], s.mx);
}

// eight 16-bit values at out + j0: one 16-byte store where the array's alignment and its end allow
__device__ __forceinline__ void depth_store8(uint16_t *out, uint32_t j0, uint32_t nbytes, const uint32_t (&v)[DEPTH_ITEMS]) {
  if (j0 >= nbytes) return;
  if (j0 + DEPTH_ITEMS <= nbytes && (((uintptr_t)out) & 15) == 0) {
    uint4 w;
    w.x = v[0] | (v[1] << 16);
    w.y = v[2] | (v[3] << 16);
    w.z = v[4] | (v[5] << 16);
    w.w = v[6] | (v[7] << 16);
    *(uint4 *)(out + j0) = w;
  } else {
#pragma unroll
    for (int k = 0; k < DEPTH_ITEMS; k++)
      if (j0 + (uint32_t)k < nbytes) out[j0 + k] = (uint16_t)v[k];
  }
}

// write: the depths go out now (not with KC_DEPTH_PER_CONTIG, whose bytes wait for the means)
__global__ void __launch_bounds__(DEPTH_TPB) kc_depth_rescan_kernel(DepthArgs a, int write) {
  __shared__ uint32_t ws[DEPTH_TPB / 64];
  __shared__ uint32_t range[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t tile0 = blockIdx.x * DEPTH_TILE, j0 = tile0 + (uint32_t)tid * DEPTH_ITEMS;
  uint32_t d[DEPTH_ITEMS];
  const uint32_t own = depth_load8(a.diff, j0, d);
  uint32_t inc = own;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    inc += lane >= o ? t : 0u;
  }
  if (lane == 63) ws[wv] = inc;
  depth_tile_range(a, tile0, range);
  __syncthreads();
  uint32_t base = (uint32_t)a.tile_sums[blockIdx.x] + inc - own;
  for (int w = 0; w < wv; w++) base += ws[w];
#pragma unroll
  for (int k = 0; k < DEPTH_ITEMS; k++) d[k] += base;  // the depth of byte j0 + k
  // the walk: head = the segment that ends at the thread's first separator, cur = the one open at its end
  DepthSeg cur = depth_seg_none(), head = depth_seg_none();
  bool sep_seen = false;
  uint32_t head_u = a.n_ctgs, u = a.n_ctgs, sep = 0xFFFFFFFFu, n_cov = 0, n_sat = 0;
  uint64_t dsum = 0;
  if (j0 < a.nbytes) {
    u = find_le(a.offs, range[0], range[1], j0);
    sep = a.offs[u + 1] - 1u;
  }
  uint32_t v[DEPTH_ITEMS];
#pragma unroll
  for (int k = 0; k < DEPTH_ITEMS; k++) {
    const uint32_t j = j0 + (uint32_t)k;
    v[k] = d[k] < 65535u ? d[k] : 65535u;
    if (j < a.nbytes) {
      if (j == sep) {  // depth 0 by construction
        if (!sep_seen) {
          head = cur;
          head_u = u;
          sep_seen = true;
        } else
          depth_seg_flush(a, u, cur);  // begun and ended in this thread
        cur = depth_seg_none();
        u++;
        sep = u < a.n_ctgs ? a.offs[u + 1] - 1u : 0xFFFFFFFFu;
      } else {
        cur.sum += d[k];
        cur.cov += d[k] ? 1u : 0u;
        cur.mn = d[k] < cur.mn ? d[k] : cur.mn;
        cur.mx = d[k] > cur.mx ? d[k] : cur.mx;
        dsum += d[k];
        n_cov += d[k] ? 1u : 0u;
        n_sat += d[k] > 65535u ? 1u : 0u;
      }
    }
  }
  if (write) depth_store8(a.depths, j0, a.nbytes, v);
  // segmented inclusive scan of the open segments: a lane that holds a separator starts one
  DepthSeg s = cur;
  wave_seg_scan(s, sep_seen, lane);
  DepthSeg carry = s.up(1);
  if (lane == 0) carry = depth_seg_none();
  if (sep_seen) depth_seg_flush(a, head_u, carry.join(head));
  if (lane == 63) depth_seg_flush(a, u, s);
  dsum = wave_sum(dsum);
  const uint64_t cs = wave_sum(((uint64_t)n_sat << 32) | n_cov);  // at most 512 each
  if (lane == 0) {
    if (dsum) atomicAdd((unsigned long long *)&a.st[DPS_DEPTH_SUM], (unsigned long long)dsum);
    if ((uint32_t)cs) atomicAdd((unsigned long long *)&a.st[DPS_COVERED], (unsigned long long)(uint32_t)cs);
    if (cs >> 32) atomicAdd((unsigned long long *)&a.st[DPS_SATURATED], (unsigned long long)(cs >> 32));
  }
}

// kc_ctg_depth: {u64 depth_sum; u32 len, covered, min_depth, max_depth, alns, mean}
__global__ void kc_depth_ctg_kernel(DepthArgs a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= a.n_ctgs) return;
  const uint32_t len = a.offs[u + 1] - 1u - a.offs[u];
  const uint64_t sum = a.csum[u];
  uint32_t mean = 0;
  if (len) {
    const uint64_t m = (sum + len / 2u) / len;
    mean = m < 65535ull ? (uint32_t)m : 65535u;
  }
  a.cmean[u] = mean;
  if (a.ctgs) {
    uint4 x, y;
    x.x = (uint32_t)sum;
    x.y = (uint32_t)(sum >> 32);
    x.z = len;
    x.w = a.ccov[u];
    y.x = len ? a.cmin[u] : 0u;
    y.y = a.cmax[u];
    y.z = a.calns[u];
    y.w = mean;
    a.ctgs[2 * (uint64_t)u] = x;
    a.ctgs[2 * (uint64_t)u + 1] = y;
  }
}

__global__ void __launch_bounds__(DEPTH_TPB) kc_depth_fill_kernel(DepthArgs a) {
  __shared__ uint32_t range[2];
  const uint32_t tile0 = blockIdx.x * DEPTH_TILE, j0 = tile0 + threadIdx.x * DEPTH_ITEMS;
  depth_tile_range(a, tile0, range);
  __syncthreads();
  if (j0 >= a.nbytes) return;
  uint32_t u = find_le(a.offs, range[0], range[1], j0);
  uint32_t sep = a.offs[u + 1] - 1u, mean = a.cmean[u];
  uint32_t v[DEPTH_ITEMS];
#pragma unroll
  for (int k = 0; k < DEPTH_ITEMS; k++) {
    const uint32_t j = j0 + (uint32_t)k;
    v[k] = mean;
    if (j == sep) {
      v[k] = 0u;
      u++;
      if (u < a.n_ctgs) {
        sep = a.offs[u + 1] - 1u;
        mean = a.cmean[u];
      } else
        sep = 0xFFFFFFFFu;
    }
  }
  depth_store8(a.depths, j0, a.nbytes, v);
}

// kc_pair_rec: {u32 aln0, aln1, insert; u8 cls; u8 pad[3]}.  a.best holds every read's best word, a.offsets the reads'.
template <bool LDS>
__global__ void __launch_bounds__(PAIR_TPB) kc_pair_classify_kernel(DepthArgs a, uint32_t max_insert, uint64_t *hist, uint4 *pairs,
                                                                      uint64_t *pst) {
  __shared__ uint32_t bins[LDS ? PAIR_LDS_BINS : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  if (LDS) {
    for (uint32_t b = (uint32_t)tid; b <= max_insert; b += PAIR_TPB) bins[b] = 0u;
    __syncthreads();
  }
  const uint64_t npairs = a.nreads >> 1;
  uint64_t n_cls[PAIR_CLASSES], isum = 0, isq = 0, with_best = 0;
#pragma unroll
  for (int k = 0; k < PAIR_CLASSES; k++) n_cls[k] = 0;
  for (uint64_t first = (uint64_t)blockIdx.x * PAIR_TPB; first < npairs; first += (uint64_t)gridDim.x * PAIR_TPB) {
    const uint64_t p = first + (uint64_t)tid;
    int cls = -1;
    uint32_t i0 = 0xFFFFFFFFu, i1 = 0xFFFFFFFFu, insert = 0;
    if (p < npairs) {
      const uint64_t w0 = a.best[2 * p], w1 = a.best[2 * p + 1];
      if (w0) i0 = 0xFFFFFFFFu - (uint32_t)w0;
      if (w1) i1 = 0xFFFFFFFFu - (uint32_t)w1;
      if (!w0 && !w1)
        cls = PAIR_NONE;
      else if (!w0 || !w1)
        cls = PAIR_ONE;
      else {
        const DepthRec b0 = depth_load(a.alns, i0), b1 = depth_load(a.alns, i1);
        if (b0.ctg != b1.ctg)
          cls = PAIR_DIFF_CTG;
        else if (b0.orient == b1.orient)
          cls = PAIR_SAME_ORIENT;
        else {
          const bool f0 = b0.orient == 0u;  // F is the orient-0 record
          const DepthRec &F = f0 ? b0 : b1, &R = f0 ? b1 : b0;
          const int64_t LR = (int64_t)(a.offsets[R.read + 1] - a.offsets[R.read]);
          const int64_t fs = (int64_t)F.cstart - (int64_t)F.rstart, rs = (int64_t)R.cstart - (int64_t)R.rstart;
          const int64_t re = (int64_t)R.cstop + (LR - (int64_t)R.rstop);
          if (rs < fs)
            cls = PAIR_EVERTED;
          else {
            insert = (uint32_t)(re - fs);  // 1 <= re - rs <= re - fs < 2^31 + 2048
            cls = insert <= max_insert ? PAIR_PROPER : PAIR_TOO_LONG;
          }
        }
      }
      if (pairs) pairs[p] = make_uint4(i0, i1, insert, (uint32_t)cls);
      if (cls == (int)PAIR_PROPER) {
        isum += insert;
        isq += (uint64_t)insert * insert;
        if (hist) {
          if (LDS)
            atomicAdd(&bins[insert], 1u);
          else
            atomicAdd((unsigned long long *)&hist[insert], 1ull);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PAIR_CLASSES; k++) n_cls[k] += wave_count(cls == k);
    with_best += wave_count(i0 != 0xFFFFFFFFu) + wave_count(i1 != 0xFFFFFFFFu);
  }
  isum = wave_sum(isum);
  isq = wave_sum(isq);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < PAIR_CLASSES; k++)
      if (n_cls[k]) atomicAdd((unsigned long long *)&pst[PRS_CLS + k], (unsigned long long)n_cls[k]);
    if (isum) atomicAdd((unsigned long long *)&pst[PRS_INSERT_SUM], (unsigned long long)isum);
    if (isq) atomicAdd((unsigned long long *)&pst[PRS_INSERT_SQ], (unsigned long long)isq);
    if (with_best) atomicAdd((unsigned long long *)&pst[PRS_WITH_BEST], (unsigned long long)with_best);
  }
  if (LDS && hist) {
    __syncthreads();
    for (uint32_t b = (uint32_t)tid; b <= max_insert; b += PAIR_TPB) {
      const uint32_t n = bins[b];
      if (n) atomicAdd((unsigned long long *)&hist[b], (unsigned long long)n);
    }
  }
}

}  // namespace kc
