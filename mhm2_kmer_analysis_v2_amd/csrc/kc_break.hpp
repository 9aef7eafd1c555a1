// kc_break.hpp -- kc_ctg_break: a contig is cut where no proper pair spans a column and the mates whose partner should lie
// across it have their partner elsewhere: a check of physical coverage behind polish or local assembly and in front of
// kc_ctg_links.  The reference holds no contig code, so the rules are this project's own (include/kcount_mi355_break.h
// states them in full, DESIGN.md section 34 the design, tests/break_model.py pins them statement by statement).
//
// Output-centric and all integers.  No workgroup waits for another; every loop's trip count comes from the input alone
// (the searches by n_ctgs and the number of breaks, the walks by 8 and 16, the tile scans by the number of tiles).
//
// Kernels, in the order of the call (the checks in front of them are kc_align_lengths_kernel, kc_depth_check_kernel and
// kc_lassm_pair_check_kernel as they stand):
//  kc_break_mark_kernel       a thread per pair: its class from its two records (break_classify), +1 / -1 for every interval
//                             that is not empty into two 32-bit difference arrays over the block, span and disc (modular).
//                             Every interval is clamped to its contig, so a contig's differences cancel at or before its
//                             separator and one unsegmented prefix sum serves the whole block (section 17).  The classes by
//                             ballots: one atomic a wave and counter.
//  kc_break_tile_sums_kernel  the sums of every tile of BREAK_TILE differences of both arrays; kc_scan_kernel<2> turns them
//                             into the tiles' bases.
//  kc_break_rescan_kernel     a tile again: base + the inclusive scan of both arrays in registers, eight consecutive columns
//                             a thread, written back in place as the exact counts; the contig of the thread's first column
//                             by section 17's search, weak decided per column against that contig's margin bounds; a weak
//                             flag per column (one 8-byte store a thread), the tile's last column that is not weak, the
//                             statistics.
//  kc_break_tile_max_kernel   one workgroup: the exclusive prefix maximum of the tiles' last columns that are not weak.
//  kc_break_runs_kernel<W>    a tile of weak flags: the thread that holds a run's last column (the next one is not weak: a
//                             contig's last column and its separator never are) knows b from itself and a from the prefix
//                             maximum -- of its own columns, the wave's, the workgroup's, the tiles before -- and decides
//                             min_run.  W = false counts the tile's breaks (kc_scan_kernel<1> gives their ranks), so that one
//                             break too many is an error before anything is stored; W = true writes {m, a, b - a} at its rank.
//  kc_break_records_kernel    a thread per input contig, per break and one more: the pieces, offsets_out, the break records
//                             (span and disc at m from the scanned arrays), the broken contigs.  The piece that begins at
//                             break r of contig u is u + r + 1; a contig's first piece is u + the breaks in front of it.
//  kc_break_gather_kernel<ES> a lane owns 16 aligned OUTPUT bytes.  The separators inserted in front of its first element
//                             by a binary search over the breaks' output positions m_r + r; a chunk without one is sixteen
//                             source bytes by aligned loads and a byte funnel shift (shuf_load16), a chunk with one goes a
//                             byte at a time.  ES = 2 gathers the depths, 0 on every inserted separator.
//  kc_break_tracks_kernel     the exact counts as saturated 16-bit tracks, eight a thread: only once the block is known to fit.
#pragma once
#include "kc_depth.hpp"
#include "kc_shuffle.hpp"

namespace kc {

constexpr int BREAK_TPB = 256;
constexpr int BREAK_ITEMS = 8;                            // consecutive columns a thread holds
constexpr uint32_t BREAK_TILE = BREAK_TPB * BREAK_ITEMS;  // T: 2048 columns a workgroup
constexpr uint32_t BREAK_ONE_MATE = 1;                    // KC_BREAK_ONE_MATE
constexpr uint32_t BREAK_NO_ALN = 0xFFFFFFFFu;
constexpr int BREAK_MAX_TPB = 1024;
static_assert(BREAK_TILE == DEPTH_TILE && BREAK_ITEMS == DEPTH_ITEMS, "depth_load8 and depth_store8 serve both");

enum { BKS_SPANNING = 0, BKS_DISC_PAIRS, BKS_ONE, BKS_NONE, BKS_DISC_MATES, BKS_EMPTY, BKS_SPAN_SUM, BKS_DISC_SUM, BKS_INTERIOR, BKS_WEAK,
       BKS_RUNS, BKS_SHORT, BKS_BREAKS, BKS_BROKEN, BKS_SCAN_SPAN, BKS_SCAN_DISC, BKS_SCAN_BREAKS, BKS_COUNT };

// ---- the per-lane rules: plain arithmetic, driven on the host against the model before any device run ------------------
struct BreakIv {
  int64_t lo, hi;  // [lo, hi); empty iff lo >= hi
};
struct BreakMate {  // what a pair's record and its read give
  uint32_t ctg, cstart, cstop, rstart, rstop, orient;
  int64_t L;
};

KC_HD BreakIv break_clamp(BreakIv v, int64_t len) { return BreakIv{v.lo < 0 ? 0 : v.lo, v.hi > len ? len : v.hi}; }

// the stretch in which a discordant mate's partner should have been found, not yet clamped
KC_HD BreakIv break_disc_iv(const BreakMate &m, uint32_t max_insert) {
  if (m.orient == 0u) {
    const int64_t s = (int64_t)m.cstart - (int64_t)m.rstart;
    return BreakIv{s, s + (int64_t)max_insert};
  }
  const int64_t e = (int64_t)m.cstop + (m.L - (int64_t)m.rstop);
  return BreakIv{e - (int64_t)max_insert, e};
}

// both mates present: true iff the pair is spanning, with [fs, re) in *span, not yet clamped
KC_HD bool break_spanning(const BreakMate &m0, const BreakMate &m1, uint32_t max_insert, BreakIv *span) {
  if (m0.ctg != m1.ctg || m0.orient == m1.orient) return false;
  const bool f0 = m0.orient == 0u;
  const BreakMate &F = f0 ? m0 : m1, &R = f0 ? m1 : m0;
  const int64_t fs = (int64_t)F.cstart - (int64_t)F.rstart, rs = (int64_t)R.cstart - (int64_t)R.rstart;
  const int64_t re = (int64_t)R.cstop + (R.L - (int64_t)R.rstop);
  if (rs < fs || re - fs > (int64_t)max_insert) return false;
  *span = BreakIv{fs, re};
  return true;
}

// column i of a contig of len bases
KC_HD bool break_interior(uint32_t i, uint32_t len, uint32_t margin) { return i >= margin && (uint64_t)i + margin < (uint64_t)len; }

// the entries of at(0 .. n) that are below x, for an at() that never decreases
template <class At>
KC_HD uint32_t break_below(uint32_t n, uint64_t x, At at) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (at(mid) < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Output element e of a block with separators inserted in front of the input positions m(0) < m(1) < ..: separator r lies at
// m(r) + r.  k: the separators below e.  Gives the input element, or -1 for an inserted separator; k moves on to e's.
template <class M>
KC_HD int64_t break_source(uint64_t e, uint32_t nb, uint32_t &k, M m) {
  while (k < nb && (uint64_t)m(k) + k < e) k++;
  if (k < nb && (uint64_t)m(k) + k == e) return -1;
  return (int64_t)(e - k);
}

#if defined(__HIPCC__)
struct BreakArgs {
  const uint32_t *offs;  // the index's n_ctgs + 1 starts
  uint32_t n_ctgs, nbytes;
  const uint4 *alns;   // kc_gap_aln
  const uint4 *pairs;  // kc_pair_rec
  const uint64_t *offsets;
  uint64_t npairs;
  uint32_t max_insert, max_span, min_disc, margin, min_run, flags;
  uint32_t *span, *disc;         // [tiles * BREAK_TILE] differences, then the exact counts
  uint64_t *tsum_span, *tsum_disc;  // [tiles]
  uint8_t *wk;                   // [tiles * BREAK_TILE] 1: weak
  uint32_t *tile_lnw, *tile_lbase;  // [tiles] 1 + the tile's last column that is not weak (0: none), and the maximum before it
  uint64_t *tile_brk;            // [tiles] breaks, then their exclusive sums
  uint4 *binfo;                  // [n_breaks] {m, a, b - a, 0} as block positions
  uint32_t n_breaks;
  uint4 *pieces, *breaks;        // the caller's, or null
  uint64_t *offsets_out;
  uint64_t *st;
};

__device__ __forceinline__ BreakMate break_mate(const BreakArgs &a, uint32_t i) {
  const DepthRec r = depth_load(a.alns, i);
  return BreakMate{r.ctg, r.cstart, r.cstop, r.rstart, r.rstop, r.orient, (int64_t)(a.offsets[r.read + 1] - a.offsets[r.read])};
}

// +1 over the clamped interval of contig u; false: it is empty.  0 <= lo < hi <= len_u: both inside [offs[u], the separator]
__device__ __forceinline__ bool break_add(const BreakArgs &a, uint32_t *diff, uint32_t u, BreakIv raw) {
  const uint32_t o = a.offs[u], len = a.offs[u + 1] - 1u - o;
  const BreakIv v = break_clamp(raw, (int64_t)len);
  if (v.lo >= v.hi) return false;
  atomicAdd(&diff[o + (uint32_t)v.lo], 1u);
  atomicAdd(&diff[o + (uint32_t)v.hi], 0xFFFFFFFFu);
  return true;
}

// the records are valid (kc_depth_check_kernel) and the pairs are (kc_lassm_pair_check_kernel)
__global__ void __launch_bounds__(BREAK_TPB) kc_break_mark_kernel(BreakArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * BREAK_TPB + threadIdx.x;
  int cls = -1;
  uint32_t mates = 0, empty = 0;
  if (p < a.npairs) {
    const uint4 pr = a.pairs[p];
    const bool has0 = pr.x != BREAK_NO_ALN, has1 = pr.y != BREAK_NO_ALN;
    if (!has0 && !has1)
      cls = BKS_NONE;
    else if (has0 && has1) {
      const BreakMate m0 = break_mate(a, pr.x), m1 = break_mate(a, pr.y);
      BreakIv sp;
      if (break_spanning(m0, m1, a.max_insert, &sp)) {
        cls = BKS_SPANNING;
        if (!break_add(a, a.span, m0.ctg, sp)) empty++;
      } else {
        cls = BKS_DISC_PAIRS;
        if (break_add(a, a.disc, m0.ctg, break_disc_iv(m0, a.max_insert))) mates++; else empty++;
        if (break_add(a, a.disc, m1.ctg, break_disc_iv(m1, a.max_insert))) mates++; else empty++;
      }
    } else {
      cls = BKS_ONE;
      if (a.flags & BREAK_ONE_MATE) {
        const BreakMate m = break_mate(a, has0 ? pr.x : pr.y);
        if (break_add(a, a.disc, m.ctg, break_disc_iv(m, a.max_insert))) mates++; else empty++;
      }
    }
  }
#pragma unroll
  for (int k = BKS_SPANNING; k <= BKS_NONE; k++) {
    const uint32_t n = wave_count(cls == k);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long *)&a.st[k], (unsigned long long)n);
  }
  wave_add(a.st, BKS_DISC_MATES, (unsigned long long)mates);
  wave_add(a.st, BKS_EMPTY, (unsigned long long)empty);
}

__global__ void __launch_bounds__(BREAK_TPB) kc_break_tile_sums_kernel(BreakArgs a) {
  __shared__ uint32_t ws[2][BREAK_TPB / 64];
  const int tid = threadIdx.x;
  const uint32_t j0 = blockIdx.x * BREAK_TILE + (uint32_t)tid * BREAK_ITEMS;
  uint32_t d[BREAK_ITEMS];
  const uint32_t s0 = wave_sum(depth_load8(a.span, j0, d)), s1 = wave_sum(depth_load8(a.disc, j0, d));
  if ((tid & 63) == 0) {
    ws[0][tid >> 6] = s0;
    ws[1][tid >> 6] = s1;
  }
  __syncthreads();
  if (tid == 0) {  // modulo 2^32, like every count
    a.tsum_span[blockIdx.x] = (uint64_t)(ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3]);
    a.tsum_disc[blockIdx.x] = (uint64_t)(ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3]);
  }
}
static_assert(BREAK_TPB == 256, "four waves a workgroup");

__device__ __forceinline__ void break_store8(uint32_t *p, const uint32_t (&v)[BREAK_ITEMS]) {
  ((uint4 *)p)[0] = make_uint4(v[0], v[1], v[2], v[3]);
  ((uint4 *)p)[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

__global__ void __launch_bounds__(BREAK_TPB) kc_break_rescan_kernel(BreakArgs a) {
  __shared__ uint32_t ws[2][BREAK_TPB / 64], wl[BREAK_TPB / 64];
  __shared__ uint32_t range[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t tile0 = blockIdx.x * BREAK_TILE, j0 = tile0 + (uint32_t)tid * BREAK_ITEMS;
  uint32_t s[BREAK_ITEMS], d[BREAK_ITEMS];
  const uint32_t own_s = depth_load8(a.span, j0, s), own_d = depth_load8(a.disc, j0, d);
  uint32_t inc_s = own_s, inc_d = own_d;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t ts = __shfl_up(inc_s, o), td = __shfl_up(inc_d, o);
    inc_s += lane >= o ? ts : 0u;
    inc_d += lane >= o ? td : 0u;
  }
  if (lane == 63) {
    ws[0][wv] = inc_s;
    ws[1][wv] = inc_d;
  }
  // the tile's first and last contig: two waves search, every thread then searches between them
  if (tid == 0) range[0] = find_le(a.offs, 0u, a.n_ctgs - 1u, tile0);
  if (tid == 64) {
    const uint32_t last = tile0 + BREAK_TILE - 1u;
    range[1] = find_le(a.offs, 0u, a.n_ctgs - 1u, last < a.nbytes ? last : a.nbytes - 1u);
  }
  __syncthreads();
  uint32_t base_s = (uint32_t)a.tsum_span[blockIdx.x] + inc_s - own_s, base_d = (uint32_t)a.tsum_disc[blockIdx.x] + inc_d - own_d;
  for (int w = 0; w < wv; w++) {
    base_s += ws[0][w];
    base_d += ws[1][w];
  }
  uint32_t u = a.n_ctgs, start = 0, sep = 0xFFFFFFFFu;
  if (j0 < a.nbytes) {
    u = find_le(a.offs, range[0], range[1], j0);
    start = a.offs[u];
    sep = a.offs[u + 1] - 1u;
  }
  uint32_t lnw = 0, n_int = 0, n_weak = 0, wlo = 0, whi = 0;
  uint64_t sum_s = 0, sum_d = 0;
#pragma unroll
  for (int k = 0; k < BREAK_ITEMS; k++) {
    const uint32_t j = j0 + (uint32_t)k;
    s[k] += base_s;  // the counts of column j; 0 on a separator and behind the block
    d[k] += base_d;
    bool weak = false;
    if (j < a.nbytes) {
      if (j == sep) {
        u++;
        start = sep + 1u;
        sep = u < a.n_ctgs ? a.offs[u + 1] - 1u : 0xFFFFFFFFu;
      } else {
        const bool in = break_interior(j - start, sep - start, a.margin);
        weak = in && s[k] <= a.max_span && d[k] >= a.min_disc;
        n_int += in ? 1u : 0u;
        sum_s += s[k];
        sum_d += d[k];
      }
    }
    if (weak) {
      n_weak++;
      if (k < 4)
        wlo |= 1u << (8 * k);
      else
        whi |= 1u << (8 * (k - 4));
    } else
      lnw = j + 1u;
  }
  break_store8(a.span + j0, s);
  break_store8(a.disc + j0, d);
  *(uint2 *)(a.wk + j0) = make_uint2(wlo, whi);
  lnw = wave_max(lnw);
  if (lane == 0) wl[wv] = lnw;
  wave_add(a.st, BKS_SPAN_SUM, (unsigned long long)sum_s);
  wave_add(a.st, BKS_DISC_SUM, (unsigned long long)sum_d);
  const int k2[2] = {BKS_INTERIOR, BKS_WEAK};
  const uint32_t mine[2] = {n_int, n_weak};
  wg_stats<2>(a.st, k2, mine);  // synchronises
  if (tid == 0) {
    uint32_t m = wl[0];
    for (int w = 1; w < BREAK_TPB / 64; w++) m = wl[w] > m ? wl[w] : m;
    a.tile_lnw[blockIdx.x] = m;
  }
}

// out[t] = the maximum of v[0 .. t), 0 for t = 0: one workgroup
__global__ void __launch_bounds__(BREAK_MAX_TPB) kc_break_tile_max_kernel(const uint32_t *v, uint32_t *out, uint64_t n) {
  __shared__ uint32_t ws[BREAK_MAX_TPB / 64];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry = 0u;
  __syncthreads();
  for (uint64_t first = 0; first < n; first += BREAK_MAX_TPB) {
    const uint64_t i = first + (uint64_t)tid;
    const uint32_t x = i < n ? v[i] : 0u;
    uint32_t inc = x;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o);
      if (lane >= o && t > inc) inc = t;
    }
    if (lane == 63) ws[wv] = inc;
    uint32_t ex = __shfl_up(inc, 1);
    if (lane == 0) ex = 0u;
    __syncthreads();
    uint32_t m = carry > ex ? carry : ex;
    for (int w = 0; w < wv; w++) m = ws[w] > m ? ws[w] : m;
    if (i < n) out[i] = m;
    __syncthreads();
    if (tid == BREAK_MAX_TPB - 1) carry = x > m ? x : m;
    __syncthreads();
  }
}

template <bool WRITE>
__global__ void __launch_bounds__(BREAK_TPB) kc_break_runs_kernel(BreakArgs a) {
  __shared__ uint32_t wm[BREAK_TPB / 64], wc[BREAK_TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t j0 = blockIdx.x * BREAK_TILE + (uint32_t)tid * BREAK_ITEMS;
  const uint2 w2 = *(const uint2 *)(a.wk + j0);
  const uint64_t bits = (uint64_t)w2.x | ((uint64_t)w2.y << 32);  // byte k: column j0 + k is weak
  // 1 + the last column that is not weak, up to and with column k: of this thread, then of everything in front of it
  uint32_t pm[BREAK_ITEMS], m = 0;
#pragma unroll
  for (int k = 0; k < BREAK_ITEMS; k++) {
    if (!((bits >> (8 * k)) & 1ull)) m = j0 + (uint32_t)k + 1u;
    pm[k] = m;
  }
  uint32_t inc = m;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o && t > inc) inc = t;
  }
  if (lane == 63) wm[wv] = inc;
  uint32_t pre = __shfl_up(inc, 1);
  if (lane == 0) pre = 0u;
  __syncthreads();
  const uint32_t before = a.tile_lbase[blockIdx.x];
  pre = before > pre ? before : pre;
  for (int w = 0; w < wv; w++) pre = wm[w] > pre ? wm[w] : pre;
  // a weak column 7 has a column behind it in the block: a contig's last column and the separators are never weak
  const bool next8 = ((bits >> 56) & 1ull) ? a.wk[j0 + BREAK_ITEMS] != 0 : false;
  uint32_t n_runs = 0, n_brk = 0;
#pragma unroll
  for (int k = 0; k < BREAK_ITEMS; k++) {
    const bool w = (bits >> (8 * k)) & 1ull, nx = k < BREAK_ITEMS - 1 ? ((bits >> (8 * (k + 1))) & 1ull) != 0 : next8;
    if (w && !nx) {  // [ra, j0 + k + 1) is a run
      const uint32_t ra = pm[k] > pre ? pm[k] : pre;
      n_runs++;
      n_brk += j0 + (uint32_t)k + 1u - ra >= a.min_run ? 1u : 0u;
    }
  }
  uint32_t cinc = n_brk;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(cinc, o);
    cinc += lane >= o ? t : 0u;
  }
  if (lane == 63) wc[wv] = cinc;
  __syncthreads();
  if (!WRITE) {
    if (tid == BREAK_TPB - 1) a.tile_brk[blockIdx.x] = (uint64_t)(wc[0] + wc[1] + wc[2] + wc[3]);
    const int k3[3] = {BKS_RUNS, BKS_SHORT, BKS_BREAKS};
    const uint32_t mine[3] = {n_runs, n_runs - n_brk, n_brk};
    wg_stats<3>(a.st, k3, mine);
  } else {
    uint32_t rank = (uint32_t)a.tile_brk[blockIdx.x] + cinc - n_brk;
    for (int w = 0; w < wv; w++) rank += wc[w];
#pragma unroll
    for (int k = 0; k < BREAK_ITEMS; k++) {
      const bool w = (bits >> (8 * k)) & 1ull, nx = k < BREAK_ITEMS - 1 ? ((bits >> (8 * (k + 1))) & 1ull) != 0 : next8;
      if (w && !nx) {
        const uint32_t ra = pm[k] > pre ? pm[k] : pre, len = j0 + (uint32_t)k + 1u - ra;
        if (len >= a.min_run && rank < a.n_breaks) a.binfo[rank++] = make_uint4(ra + len / 2u, ra, len, 0u);
      }
    }
  }
}

// kc_break_piece {ctg, start, len, flags}; kc_break_rec {ctg, pos, run_start, run_len, span, disc, piece, pad}
__global__ void __launch_bounds__(BREAK_TPB) kc_break_records_kernel(BreakArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * BREAK_TPB + threadIdx.x;
  const uint32_t nb = a.n_breaks;
  const uint4 *bi = a.binfo;
  bool broken = false;
  if (t < a.n_ctgs) {  // a contig's first piece
    const uint32_t u = (uint32_t)t, o = a.offs[u], e = a.offs[u + 1] - 1u;
    const uint32_t r0 = break_below(nb, (uint64_t)o, [bi](uint32_t r) { return (uint64_t)bi[r].x; });
    const bool cut = r0 < nb && bi[r0].x < e;
    const uint64_t q = (uint64_t)u + r0;
    broken = cut;
    if (a.pieces) a.pieces[q] = make_uint4(u, 0u, (cut ? bi[r0].x : e) - o, cut ? 2u : 0u);
    if (a.offsets_out) a.offsets_out[q] = (uint64_t)o + r0;
  } else if (t < (uint64_t)a.n_ctgs + nb) {  // the piece that begins at a break
    const uint32_t r = (uint32_t)(t - a.n_ctgs);
    const uint4 b = bi[r];
    const uint32_t u = find_le(a.offs, 0u, a.n_ctgs - 1u, b.x), o = a.offs[u], e = a.offs[u + 1] - 1u;
    const bool cut = r + 1u < nb && bi[r + 1u].x < e;
    const uint64_t q = (uint64_t)u + r + 1u;
    if (a.pieces) a.pieces[q] = make_uint4(u, b.x - o, (cut ? bi[r + 1u].x : e) - b.x, 1u | (cut ? 2u : 0u));
    if (a.offsets_out) a.offsets_out[q] = (uint64_t)b.x + r + 1u;
    if (a.breaks) {
      a.breaks[2 * (uint64_t)r] = make_uint4(u, b.x - o, b.y - o, b.z);
      const bool in = b.x < a.nbytes;  // always: m is a column
      a.breaks[2 * (uint64_t)r + 1] = make_uint4(in ? a.span[b.x] : 0u, in ? a.disc[b.x] : 0u, (uint32_t)q, 0u);
    }
  } else if (t == (uint64_t)a.n_ctgs + nb && a.offsets_out)
    a.offsets_out[t] = (uint64_t)a.nbytes + nb;
  const uint32_t n = wave_count(broken);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long *)&a.st[BKS_BROKEN], (unsigned long long)n);
}

struct BreakCopy {
  const uint8_t *src;  // elements of ES bytes
  uint8_t *dst;
  const uint4 *binfo;
  uint32_t nb;
  uint64_t total, src_total;  // in elements
};

// Thread t owns dst's bytes [16 t - mis, 16 t - mis + 16) cut to [0, ES total): mis = dst's address & 15, so every whole chunk
// is an aligned 16-byte store.  total >= 1 (the host launches nothing otherwise); ES = 2: dst is 2-byte aligned.
template <int ES>
__global__ void __launch_bounds__(BREAK_TPB) kc_break_gather_kernel(BreakCopy a) {
  const int64_t mis = (int64_t)((uintptr_t)a.dst & 15u), tb = (int64_t)ES * (int64_t)a.total;
  const int64_t p0 = (int64_t)(((uint64_t)blockIdx.x * BREAK_TPB + threadIdx.x) * 16) - mis;
  if (p0 >= tb) return;
  const int64_t from = p0 < 0 ? 0 : p0, to = p0 + 16 < tb ? p0 + 16 : tb;
  const uint4 *bi = a.binfo;
  const auto m = [bi](uint32_t r) { return bi[r].x; };
  const uint64_t e0 = (uint64_t)(from / ES), e1 = (uint64_t)((to + ES - 1) / ES);
  uint32_t k = break_below(a.nb, e0, [bi](uint32_t r) { return (uint64_t)bi[r].x + r; });  // separators below the first element
  const bool whole = to - from == 16, none = k >= a.nb || (uint64_t)bi[k].x + k >= e1;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const uintptr_t src_lo = (uintptr_t)a.src, src_hi = src_lo + (uintptr_t)ES * a.src_total;
  bool done = false;
  if (whole && none) done = shuf_load16(src_lo, src_hi, src_lo + (uintptr_t)(from - (int64_t)ES * k), w);
  if (!done) {  // an end of the block, an inserted separator, or aligned loads that would leave the source array
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      uint32_t c = 0;
      if (p >= from && p < to) {
        const int64_t at = break_source((uint64_t)(p / ES), a.nb, k, m);
        c = at < 0 ? (ES == 1 ? (uint32_t)'_' : 0u) : (uint64_t)at < a.src_total ? a.src[at * ES + (p % ES)] : 0u;  // always inside
      }
      w[j >> 2] |= c << (8 * (j & 3));
    }
  }
  if (whole)
    *(uint4 *)(a.dst + p0) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      if (p >= from && p < to) a.dst[p] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

__global__ void __launch_bounds__(BREAK_TPB) kc_break_tracks_kernel(const uint32_t *v, uint16_t *out, uint32_t nbytes) {
  const uint32_t j0 = (blockIdx.x * BREAK_TPB + threadIdx.x) * BREAK_ITEMS;
  if (j0 >= nbytes) return;
  const uint4 x = ((const uint4 *)(v + j0))[0], y = ((const uint4 *)(v + j0))[1];
  const uint32_t r[BREAK_ITEMS] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
  uint32_t s[BREAK_ITEMS];
#pragma unroll
  for (int k = 0; k < BREAK_ITEMS; k++) s[k] = r[k] < 65535u ? r[k] : 65535u;
  depth_store8(out, j0, nbytes, s);
}
#endif  // __HIPCC__

}  // namespace kc
