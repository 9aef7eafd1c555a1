// kc_polish.hpp -- kc_ctg_polish: every column of the indexed block rewritten to the clear winner of the pileup of the reads'
// gapped records.  The reference holds no contig or alignment code (no Alns, no pileup in src/), so the rules are this
// project's own definition (include/kcount_mi355_polish.h states them in full, DESIGN.md section 33, pinned statement by
// statement by tests/polish_model.py); no parity with MetaHipMer is claimed.
//
// Rules in short:
//  * Validity, the filter and a read's best record are kc_depth.hpp's; read < nreads and rstop <= L(read) always apply.
//  * A record is PLACED iff it passes the filter (and is its read's best with POLISH_BEST_ONLY), lies on one diagonal
//    (cstop - cstart == rstop - rstart) and differs from the contig at no more than max_mismatches of its columns, counted
//    here where both codes are below 4 (the record's own field is not read).
//  * It votes at i in [e_lo, span - e_hi) (kc_depth.hpp's clipping): +1 to cnt[cstart + i][code of R'[rstart + i]] for a
//    code below 4 whose quality passes min_qual.
//  * A column with tot >= min_depth, top > second and top * 1000 >= min_permille * tot becomes "ACGT"[winner] where that
//    differs from what it holds; every other byte, and every separator, is copied.
//
// The design is output-centric: no counter of a column ever exists in global memory (16 bytes a column would be 16 GB for
// a 988 MB block).  The records are sorted by the block position of their first column; a workgroup owns a tile of
// POLISH_TILE block bytes, keeps the tile's 4 x u32 counters in LDS and reads the records that can reach into it.
//
// Kernels:
//  kc_polish_place_kernel     a wave per record: its class, for a candidate the mismatches along the diagonal -- a lane takes
//                             16 columns: the contig's bytes and the read's as two aligned 16-byte loads and a funnel shift
//                             each (shuf_load16, kc_shuffle.hpp), the read reversed in registers for orient 1 -- and the
//                             32-bit key offs[ctg] + cstart (POLISH_NO_KEY for a record that is not placed).
//  (the sort)                 kc_sort.hpp's hist and scatter passes and kc_scan_kernel<1> over the key's significant bits, as
//                             kc_api_shuffle.hpp uses them; no instance of either is added.
//  kc_polish_tile_kernel<W>   a workgroup per tile.  It zeroes its counters, finds by two binary searches the sorted records
//                             with a key in [tile_lo - (ALIGN_MAX_READ_LEN - 1), tile_hi), and its four waves take them in
//                             turn: a lane loads its 16 bases (and qualities) of R' where they fall in the tile and adds
//                             their votes with non-returning LDS atomics.  After the barrier the first POLISH_TILE / 16
//                             lanes own 16 aligned bytes each and decide their columns.  <0> (count) stores a lane's and the
//                             tile's number of changed columns and nothing else; <1> (write) stores the 16 bytes in one
//                             store, the saturated counts, the fix records at their scanned places, and adds the per-contig
//                             and global counters: a wave that lies in one contig adds its sums once, a lane that crosses a
//                             separator adds its own.  Integer adds only: the result does not depend on arrival order.
// No loop depends on another thread's progress: every trip count comes from the input.  A tile under a very deep contig
// does proportionally more work (its waves walk every record that reaches it); splitting such tiles is not done.
// The per-lane work is written as functions of (tile, lane) with no wave intrinsic in them, so that a host compiler can
// build them and run them under sanitizers against the model.
#pragma once
#include "kc_depth.hpp"
#include "kc_shuffle.hpp"

namespace kc {

constexpr int POLISH_TPB = 256;
constexpr int POLISH_WAVES = POLISH_TPB / 64;
constexpr uint32_t POLISH_TILE = 1024;                 // block bytes a workgroup: 4 x u32 a column, 16 KiB of LDS
constexpr int POLISH_OUT_LANES = POLISH_TILE / 16;     // the lanes that own 16 output bytes
constexpr uint32_t POLISH_NO_KEY = 0xFFFFFFFFu;
constexpr uint32_t POLISH_BEST_ONLY = 1;
constexpr uint32_t POLISH_MAX_PERMILLE = 1000, POLISH_MAX_QUAL = 255;
static_assert(ALIGN_MAX_READ_LEN == 64 * 16, "a wave's lanes take a record's 16-byte chunks in one round");
static_assert(POLISH_OUT_LANES <= POLISH_TPB && POLISH_OUT_LANES % 64 == 0, "whole waves decide");

enum { PLS_NONE = 0, PLS_FILTERED, PLS_NOT_BEST, PLS_UNEQUAL, PLS_DIVERGENT, PLS_PLACED, PLS_VOTES, PLS_UNCOVERED, PLS_THIN, PLS_DISPUTED,
       PLS_CONFIRMED, PLS_CHANGED, PLS_FILLED, PLS_FIXES, PLS_SORT_TOTAL, PLS_COUNT };
// a contig's accumulators, laid out as kc_polish_ctg: u64 votes; u32 placed, changed, filled, disputed, thin, uncovered
enum { PLC_PLACED = 2, PLC_CHANGED, PLC_FILLED, PLC_DISPUTED, PLC_THIN, PLC_UNCOVERED, PLC_WORDS };

struct PolishArgs {
  const uint8_t *seqs;   // the index's block
  const uint32_t *offs;  // its n_ctgs + 1 starts
  uint32_t n_ctgs, nbytes;
  const uint8_t *bases, *quals;  // the reads; quals null: no gate
  const uint64_t *offsets;
  uint64_t total;  // the reads' bytes
  const uint4 *alns;
  uint64_t n_alns;
  uint32_t min_score, min_len, edge_clip, max_mismatches, min_depth, min_permille, min_qual, flags;
  int32_t qual_offset;
  const uint64_t *best;  // [nreads] with POLISH_BEST_ONLY
  uint64_t *keys;        // [n_alns]: the place kernel's
  const uint64_t *skeys; // the sorted keys and where they came from (null: the identity)
  const uint32_t *perm;
  uint8_t *out;          // [nbytes]
  uint16_t *counts;      // [nbytes * 4] or null
  uint32_t *cacc;        // [n_ctgs * PLC_WORDS]
  uint8_t *lane_changed; // [tiles * POLISH_OUT_LANES], with fixes
  uint64_t *tile_changed;  // [tiles]: the count pass's, scanned
  const uint64_t *tile_base;
  uint4 *fixes;          // kc_polish_fix or null
  uint64_t *st;
};

// The sixteen bytes [at, at + 16) of base[0, total) as four dwords, zero outside the array: shuf_load16 where its aligned
// loads stay inside, byte loads at the array's ends.
__device__ __forceinline__ void polish_load16(const uint8_t *base, uint64_t total, int64_t at, uint32_t (&w)[4]) {
  if (at >= 0 && shuf_load16((uintptr_t)base, (uintptr_t)base + total, (uintptr_t)base + (uint64_t)at, w)) return;
  w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int64_t j = at + k;
    if (j >= 0 && (uint64_t)j < total) w[k >> 2] |= (uint32_t)base[j] << (8 * (k & 3));
  }
}

// the bytes that stand behind R'[p, p + 16) in `src` (bases or quals) of the read at [roff, roff + L), in R's order: for
// orient 1 the sixteen bytes that end at L - 1 - p, reversed in registers
__device__ __forceinline__ void polish_read16(const uint8_t *src, uint64_t total, uint64_t roff, uint32_t L, uint32_t orient, uint32_t p,
                                              uint32_t (&w)[4]) {
  if (!orient) {
    polish_load16(src, total, (int64_t)(roff + p), w);
    return;
  }
  uint32_t t[4];
  polish_load16(src, total, (int64_t)roff + (int64_t)L - 16 - (int64_t)p, t);
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = __builtin_bswap32(t[3 - j]);
}

__device__ __forceinline__ uint32_t polish_byte(const uint32_t (&w)[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }

// the code of R' behind a byte of the read
__device__ __forceinline__ uint32_t polish_code(uint32_t byte, uint32_t orient) {
  const uint32_t c = base_code4(byte);
  return (orient && c < 4u) ? 3u - c : c;
}

// lane's share of m: the columns [16 lane, 16 lane + 16) of the record's diagonal at which both codes are bases and differ
__device__ __forceinline__ uint32_t polish_lane_mismatches(const PolishArgs &a, const DepthRec &r, int lane) {
  const uint32_t span = r.cstop - r.cstart, i0 = 16u * (uint32_t)lane;
  if (i0 >= span) return 0u;
  const uint64_t roff = a.offsets[r.read];
  const uint32_t L = (uint32_t)(a.offsets[r.read + 1] - roff);
  uint32_t cw[4], rw[4];
  polish_load16(a.seqs, a.nbytes, (int64_t)a.offs[r.ctg] + (int64_t)r.cstart + (int64_t)i0, cw);
  polish_read16(a.bases, a.total, roff, L, r.orient, r.rstart + i0, rw);
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t cc = base_code4(polish_byte(cw, k)), rc = polish_code(polish_byte(rw, k), r.orient);
    m += (i0 + (uint32_t)k < span && cc < 4u && rc < 4u && cc != rc) ? 1u : 0u;
  }
  return m;
}

// the class of a record short of the mismatches: PLS_PLACED stands for "count them"
__device__ __forceinline__ int polish_class(const PolishArgs &a, const DepthRec &r, uint64_t i) {
  if (r.kind == GAP_KIND_NONE) return PLS_NONE;
  if (!(r.score >= a.min_score && r.cstop - r.cstart >= a.min_len)) return PLS_FILTERED;
  if ((a.flags & POLISH_BEST_ONLY) && a.best[r.read] != depth_best_word(r.score, i)) return PLS_NOT_BEST;
  if (r.cstop - r.cstart != r.rstop - r.rstart) return PLS_UNEQUAL;
  return PLS_PLACED;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(POLISH_TPB) kc_polish_place_kernel(PolishArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t i = (uint64_t)blockIdx.x * POLISH_WAVES + (threadIdx.x >> 6);
  int cls = -1;  // the whole wave's
  if (i < a.n_alns) {
    const DepthRec r = depth_load(a.alns, i);
    cls = polish_class(a, r, i);
    if (cls == PLS_PLACED && wave_sum(polish_lane_mismatches(a, r, lane)) > a.max_mismatches) cls = PLS_DIVERGENT;
    if (lane == 0) {
      a.keys[i] = cls == PLS_PLACED ? (uint64_t)(a.offs[r.ctg] + r.cstart) : (uint64_t)POLISH_NO_KEY;
      if (cls == PLS_PLACED) atomicAdd(&a.cacc[(uint64_t)r.ctg * PLC_WORDS + PLC_PLACED], 1u);
    }
  }
  const int kinds[6] = {PLS_NONE, PLS_FILTERED, PLS_NOT_BEST, PLS_UNEQUAL, PLS_DIVERGENT, PLS_PLACED};
  uint32_t mine[6];
#pragma unroll
  for (int k = 0; k < 6; k++) mine[k] = (lane == 0 && cls == kinds[k]) ? 1u : 0u;
  wg_stats<6>(a.st, kinds, mine);
}
#endif

// ---- the tile ----------------------------------------------------------------------------------------------------------
// the first s in [0, n) with keys[s] >= x, n where there is none
__device__ __forceinline__ uint64_t polish_lower_bound(const uint64_t *keys, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void polish_lds_add(uint32_t *p) {
#if defined(__HIPCC__)
  atomicAdd(p, 1u);  // the result is not used: a non-returning ds_add_u32
#else
  ++*p;
#endif
}

// Sorted record s: the votes of lane's 16 columns of its diagonal that fall into the tile [tile_lo, tile_hi), into cnt
// (4 counters a column of the tile).
__device__ __forceinline__ void polish_vote(const PolishArgs &a, uint32_t *cnt, uint32_t tile_lo, uint32_t tile_hi, uint64_t s, int lane) {
  const int64_t key = (int64_t)a.skeys[s];
  const DepthRec r = depth_load(a.alns, a.perm ? (uint64_t)a.perm[s] : s);
  const uint32_t o = a.offs[r.ctg], len = a.offs[r.ctg + 1] - 1u - o;
  // i in [lo, hi): inside the clipped span and inside the tile
  int64_t lo = r.cstart > 0u ? (int64_t)a.edge_clip : 0;
  int64_t hi = (int64_t)(r.cstop - r.cstart) - (r.cstop < len ? (int64_t)a.edge_clip : 0);
  const int64_t i0 = 16 * (int64_t)lane;
  if (lo < (int64_t)tile_lo - key) lo = (int64_t)tile_lo - key;
  if (hi > (int64_t)tile_hi - key) hi = (int64_t)tile_hi - key;
  if (lo < i0) lo = i0;
  if (hi > i0 + 16) hi = i0 + 16;
  if (lo >= hi) return;
  const uint64_t roff = a.offsets[r.read];
  const uint32_t L = (uint32_t)(a.offsets[r.read + 1] - roff);
  const bool gate = a.quals && a.min_qual;
  uint32_t rw[4], qw[4] = {0u, 0u, 0u, 0u};
  polish_read16(a.bases, a.total, roff, L, r.orient, r.rstart + (uint32_t)i0, rw);
  if (gate) polish_read16(a.quals, a.total, roff, L, r.orient, r.rstart + (uint32_t)i0, qw);
  // the chunk's bytes as two 64-bit halves, so that a loop over the voting bytes alone needs no register indexing: 150-base
  // reads leave most chunks of a tile's edge records a few bytes, and the unrolled sixteen cost sixteen more registers
  const uint64_t r_lo = rw[0] | ((uint64_t)rw[1] << 32), r_hi = rw[2] | ((uint64_t)rw[3] << 32);
  const uint64_t q_lo = qw[0] | ((uint64_t)qw[1] << 32), q_hi = qw[2] | ((uint64_t)qw[3] << 32);
  const int64_t col0 = key + i0 - (int64_t)tile_lo;  // the tile column of the chunk's first base; 0 <= col0 + k < POLISH_TILE where it votes
#pragma unroll 1
  for (int k = (int)(lo - i0); k < (int)(hi - i0); k++) {
    const int sh = 8 * (k & 7);
    const uint32_t b = polish_code((uint32_t)((k < 8 ? r_lo : r_hi) >> sh) & 0xFFu, r.orient);
    const bool q_ok = !gate || (int32_t)((uint32_t)((k < 8 ? q_lo : q_hi) >> sh) & 0xFFu) - a.qual_offset >= (int32_t)a.min_qual;
    if (b < 4u && q_ok) polish_lds_add(&cnt[(uint32_t)(col0 + k) * 4u + b]);
  }
}

// what a lane of the decision adds up for the contig it stands in, and for the call
struct PolishAcc {
  uint64_t votes;
  uint32_t changed, filled, disputed, thin, uncovered, confirmed;
};

__device__ __forceinline__ void polish_acc_flush(const PolishArgs &a, uint32_t u, const PolishAcc &s) {
#if defined(__HIPCC__)
  if (u >= a.n_ctgs) return;
  uint32_t *p = a.cacc + (uint64_t)u * PLC_WORDS;
  if (s.votes) atomicAdd((unsigned long long *)p, (unsigned long long)s.votes);
  if (s.changed) atomicAdd(p + PLC_CHANGED, s.changed);
  if (s.filled) atomicAdd(p + PLC_FILLED, s.filled);
  if (s.disputed) atomicAdd(p + PLC_DISPUTED, s.disputed);
  if (s.thin) atomicAdd(p + PLC_THIN, s.thin);
  if (s.uncovered) atomicAdd(p + PLC_UNCOVERED, s.uncovered);
#else
  if (u >= a.n_ctgs) return;
  uint32_t *p = a.cacc + (uint64_t)u * PLC_WORDS;
  *(uint64_t *)p += s.votes;
  p[PLC_CHANGED] += s.changed, p[PLC_FILLED] += s.filled, p[PLC_DISPUTED] += s.disputed, p[PLC_THIN] += s.thin, p[PLC_UNCOVERED] += s.uncovered;
#endif
}

// A lane's 16 columns [j0, j0 + 16) of the block, j0 = tile_lo + 16 t < nbytes: the decisions from the tile's counters.
// WRITE false: returns the number of changed columns and stores nothing.  WRITE true: out, counts, the fixes from slot
// `fix_at` on; `tot` takes the lane's total for the call, `acc`
// what is open for contig `u` at its end, `crossed` whether it met a separator.  u0: the contig of j0.
template <bool WRITE>
__device__ __forceinline__ uint32_t polish_decide(const PolishArgs &a, const uint32_t *cnt, uint32_t tile_lo, int t, uint32_t u0, uint64_t fix_at,
                                                  PolishAcc &tot, PolishAcc &acc, uint32_t &u, bool &crossed) {
  const uint32_t j0 = tile_lo + 16u * (uint32_t)t;
  uint32_t cw[4];
  polish_load16(a.seqs, a.nbytes, (int64_t)j0, cw);
  // the sixteen bytes as two 64-bit halves, in and out: the loop over them is not unrolled (sixteen copies of it cost the
  // kernel its 64 registers), so a byte is a shift of a half, not an indexed register
  const uint64_t c_lo = cw[0] | ((uint64_t)cw[1] << 32), c_hi = cw[2] | ((uint64_t)cw[3] << 32);
  uint64_t o_lo = c_lo, o_hi = c_hi;
  u = u0;
  uint32_t sep = a.offs[u + 1] - 1u, n_changed = 0;
  const uint4 *c4 = (const uint4 *)(cnt + 64u * (uint32_t)t);
  const bool counts16 = WRITE && a.counts && (((uintptr_t)a.counts) & 15) == 0 && j0 + 16u <= a.nbytes;
  uint4 pair = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
  for (int k = 0; k < 16; k++) {
    const uint32_t j = j0 + (uint32_t)k;
    const int sh = 8 * (k & 7);
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (j < a.nbytes) {
      if (j == sep) {  // no vote reaches a separator: cstop <= len_u
        if (WRITE) {
          polish_acc_flush(a, u, acc);
          acc = PolishAcc{0ull, 0u, 0u, 0u, 0u, 0u, 0u};
          crossed = true;
        }
        u++;
        sep = u < a.n_ctgs ? a.offs[u + 1] - 1u : 0xFFFFFFFFu;
      } else {
        c = c4[k];
        const uint32_t old = (uint32_t)((k < 8 ? c_lo : c_hi) >> sh) & 0xFFu, cur = base_code4(old);
        const uint32_t sum = c.x + c.y + c.z + c.w;  // at most 2^32 - 1 records: exact
        // the winner: the lowest code that holds the greatest count; second: the greatest of the other three
        uint32_t w = 0, top = c.x;
        if (c.y > top) w = 1, top = c.y;
        if (c.z > top) w = 2, top = c.z;
        if (c.w > top) w = 3, top = c.w;
        uint32_t second = 0;
        if (w != 0 && c.x > second) second = c.x;
        if (w != 1 && c.y > second) second = c.y;
        if (w != 2 && c.z > second) second = c.z;
        if (w != 3 && c.w > second) second = c.w;
        const bool uncovered = sum == 0u, thin = !uncovered && sum < a.min_depth;
        const bool disputed = !uncovered && !thin && (top == second || (uint64_t)top * 1000ull < (uint64_t)a.min_permille * (uint64_t)sum);
        const bool decided = !uncovered && !thin && !disputed, change = decided && w != cur;
        n_changed += change ? 1u : 0u;
        if (WRITE) {
          acc.votes += sum, tot.votes += sum;
          acc.uncovered += uncovered, tot.uncovered += uncovered;
          acc.thin += thin, tot.thin += thin;
          acc.disputed += disputed, tot.disputed += disputed;
          tot.confirmed += decided && !change;
          acc.changed += change, tot.changed += change;
          acc.filled += change && cur == 4u, tot.filled += change && cur == 4u;
          if (change) {
            const uint32_t neu = code_letter(w);
            const uint64_t flip = (uint64_t)(neu ^ old) << sh;
            if (k < 8)
              o_lo ^= flip;
            else
              o_hi ^= flip;
            if (a.fixes) {
              const uint32_t top16 = top < 65535u ? top : 65535u, sum16 = sum < 65535u ? sum : 65535u;
              a.fixes[fix_at++] = make_uint4(j, u, old | (neu << 8) | (top16 << 16), sum16);
            }
          }
        }
      }
    }
    if (WRITE && a.counts) {
      const uint32_t x = c.x < 65535u ? c.x : 65535u, y = c.y < 65535u ? c.y : 65535u, z = c.z < 65535u ? c.z : 65535u,
                     v = c.w < 65535u ? c.w : 65535u;
      if (counts16) {  // two columns a 16-byte store
        if (k & 1) {
          pair.z = x | (y << 16), pair.w = z | (v << 16);
          *(uint4 *)(a.counts + 4ull * (uint64_t)(j - 1u)) = pair;
        } else
          pair.x = x | (y << 16), pair.y = z | (v << 16);
      } else if (j < a.nbytes) {
        uint16_t *p = a.counts + 4ull * (uint64_t)j;
        p[0] = (uint16_t)x, p[1] = (uint16_t)y, p[2] = (uint16_t)z, p[3] = (uint16_t)v;
      }
    }
  }
  if (WRITE) {
    if (j0 + 16u <= a.nbytes && (((uintptr_t)a.out) & 15) == 0)
      *(uint4 *)(a.out + j0) = make_uint4((uint32_t)o_lo, (uint32_t)(o_lo >> 32), (uint32_t)o_hi, (uint32_t)(o_hi >> 32));
    else {
#pragma unroll 1
      for (int k = 0; k < 16; k++)
        if (j0 + (uint32_t)k < a.nbytes) a.out[j0 + k] = (uint8_t)((k < 8 ? o_lo : o_hi) >> (8 * (k & 7)));
    }
  }
  return n_changed;
}

#if defined(__HIPCC__)
struct PolishAccWave {
  PolishAcc s;
  __device__ __forceinline__ PolishAccWave across(int o) const {
    return PolishAccWave{PolishAcc{__shfl_xor(s.votes, o), __shfl_xor(s.changed, o), __shfl_xor(s.filled, o), __shfl_xor(s.disputed, o),
                                   __shfl_xor(s.thin, o), __shfl_xor(s.uncovered, o), __shfl_xor(s.confirmed, o)}};
  }
  __device__ __forceinline__ PolishAccWave join(const PolishAccWave &y) const {
    return PolishAccWave{PolishAcc{s.votes + y.s.votes, s.changed + y.s.changed, s.filled + y.s.filled, s.disputed + y.s.disputed, s.thin + y.s.thin,
                                   s.uncovered + y.s.uncovered, s.confirmed + y.s.confirmed}};
  }
};

template <int WRITE>
__global__ void __launch_bounds__(POLISH_TPB) kc_polish_tile_kernel(PolishArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t cnt[POLISH_TILE * 4];
  __shared__ uint64_t recs[2];
  __shared__ uint32_t range[2];
  __shared__ uint32_t ws[POLISH_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t tile_lo = blockIdx.x * POLISH_TILE;
  const uint32_t tile_hi = a.nbytes - tile_lo < POLISH_TILE ? a.nbytes : tile_lo + POLISH_TILE;
#pragma unroll
  for (int j = 0; j < (int)(POLISH_TILE * 4 / 4 / POLISH_TPB); j++) ((uint4 *)cnt)[j * POLISH_TPB + tid] = make_uint4(0u, 0u, 0u, 0u);
  // the records that reach into the tile start at most a read's length less one ahead of it (thread 0, thread 64), and
  // the tile's first and last contig (thread 128, thread 192): four waves
  if (tid == 0) recs[0] = polish_lower_bound(a.skeys, a.n_alns, tile_lo > (uint32_t)(ALIGN_MAX_READ_LEN - 1) ? tile_lo - (ALIGN_MAX_READ_LEN - 1) : 0u);
  if (tid == 64) recs[1] = polish_lower_bound(a.skeys, a.n_alns, tile_hi);
  if (tid == 128) range[0] = find_le(a.offs, 0u, a.n_ctgs - 1u, tile_lo);
  if (tid == 192) range[1] = find_le(a.offs, 0u, a.n_ctgs - 1u, tile_hi - 1u);
  __syncthreads();
  for (uint64_t s = recs[0] + (uint64_t)wv; s < recs[1]; s += POLISH_WAVES) polish_vote(a, cnt, tile_lo, tile_hi, s, lane);
  __syncthreads();
  const uint32_t j0 = tile_lo + 16u * (uint32_t)tid;
  const bool mine = tid < POLISH_OUT_LANES && j0 < a.nbytes;
  uint32_t u0 = 0;
  if (mine) u0 = find_le(a.offs, range[0], range[1], j0);
  PolishAcc tot{0ull, 0u, 0u, 0u, 0u, 0u, 0u}, acc = tot;
  uint32_t u = a.n_ctgs;
  bool crossed = false;
  if (!WRITE) {
    const uint32_t n = mine ? polish_decide<false>(a, cnt, tile_lo, tid, u0, 0, tot, acc, u, crossed) : 0u;
    if (tid < POLISH_OUT_LANES) a.lane_changed[(uint64_t)blockIdx.x * POLISH_OUT_LANES + tid] = (uint8_t)n;
    const uint32_t sum = wave_sum(n);
    if (lane == 0) ws[wv] = sum;
    __syncthreads();
    if (tid == 0) {
      uint32_t all = 0;
      for (int w = 0; w < POLISH_WAVES; w++) all += ws[w];
      a.tile_changed[blockIdx.x] = all;
    }
    return;
  }
  uint64_t fix_at = 0;
  if (a.fixes) {  // the lane's place among the fixes: the tile's scanned base and the lanes ahead of it
    const uint32_t n = tid < POLISH_OUT_LANES ? a.lane_changed[(uint64_t)blockIdx.x * POLISH_OUT_LANES + tid] : 0u;
    uint32_t inc = n;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t x = __shfl_up(inc, o);
      inc += lane >= o ? x : 0u;
    }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    fix_at = a.tile_base[blockIdx.x >> LINK_SCAN_SHIFT] + a.tile_changed[blockIdx.x] + (inc - n);
    for (int w = 0; w < wv; w++) fix_at += ws[w];
  }
  if (mine) polish_decide<true>(a, cnt, tile_lo, tid, u0, fix_at, tot, acc, u, crossed);
  if (wv < POLISH_OUT_LANES / 64) {
    // a wave that stands in one contig adds its sums once; else every lane its own
    const uint32_t first_u = __shfl(u, 0);
    const bool uniform = !__any(mine && (crossed || u != first_u));
    if (uniform) {
      const PolishAccWave s = wave_join(PolishAccWave{acc});
      if (lane == 0) polish_acc_flush(a, first_u, s.s);
    } else if (mine)
      polish_acc_flush(a, u, acc);
  }
  wave_add(a.st, PLS_VOTES, (unsigned long long)tot.votes);
  const int kinds[6] = {PLS_UNCOVERED, PLS_THIN, PLS_DISPUTED, PLS_CONFIRMED, PLS_CHANGED, PLS_FILLED};
  const uint32_t mine6[6] = {tot.uncovered, tot.thin, tot.disputed, tot.confirmed, tot.changed, tot.filled};
  wg_stats<6>(a.st, kinds, mine6);
}
#endif

}  // namespace kc
