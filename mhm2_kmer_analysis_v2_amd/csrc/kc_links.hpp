// kc_links.hpp -- the links between contig ends (kc_ctg_links): splints, where one read is aligned across two contigs, and
// spans, where the two mates of a pair have their best records on different contigs -- the adjacency list of the contig
// graph, the first half of scaffolding.  The reference holds no code for it (no cgraph, no Alns, no scaffolding in src/),
// so the rules are this project's own definition (pinned statement by statement by
// tests/links_model.py); no parity with MetaHipMer is claimed.  include/kcount_mi355.h states the rules in full.
//
// Kernels, in the order of the call (the checks in front of them are kc_align_lengths_kernel, kc_depth_check_kernel and
// kc_lassm_pair_check_kernel):
//  kc_link_group_kernel<W>   a thread per record, run twice.  W = false counts the passing records of every read (one
//                            64-bit atomic a record) and the call's record statistics; the two-level scan below turns the
//                            counts into the reads' first slots; W = true takes a slot through the read's cursor (which
//                            ends as the read's count) and writes what the splint rule needs of the record as one
//                            16-byte store: {qs | qe << 16, ctg << 1 | orient,
//                            e as a leaver, e as an enterer} (LINK_NO_END: it does not reach that end).  The order inside
//                            a read is left free: the rule is over all ordered pairs.
//  kc_link_cands_kernel<W>   a thread per read (its splints: every ordered pair of its slots) and, behind the reads, a
//                            thread per pair (its span), run twice: W = false counts a thread's candidates and the
//                            statistics (wave sums, then one atomic a workgroup of 1024 threads and counter), the
//                            two-level scan makes the counts positions, W = true writes.  A candidate is
//                            written ONCE IN EACH DIRECTION -- the keys from << 32 | to and to << 32 | from, one 16-byte
//                            store -- beside one 32-bit payload, kind << 24 | (gap + 65536).  So the sorted items are the
//                            directed records' supporters as they stand, and a link's two records need no second sort.
//  kc_link_tile_scan_kernel  the first level of the scans over the reads and over the threads: a workgroup per tile of
//                            LINK_SCAN_TILE counts scans it in place and leaves the tile's total; kc_scan_kernel<1>
//                            (kc_scan.hpp, one workgroup: made for tile sums) turns the totals into the tiles' bases, and a
//                            reader adds base[i / LINK_SCAN_TILE] to item i.  The one-workgroup scan over every read took
//                            three fifths of the call's kernel time before.
//  kc_sort_hist_kernel / kc_sort_scatter_kernel (kc_sort.hpp)  the radix passes over the significant bits only:
//                            b = the bits of 2 n_ctgs - 1, `to` in bits [0, b) and `from` in bits [32, 32 + b).
//  kc_link_heads_kernel      a workgroup per tile of LINK_TILE sorted items: the heads of runs (an item whose key differs
//                            from the one before it) in the tile; kc_scan_kernel<1> makes them the tiles' first run.
//  kc_link_reduce_kernel     a thread per sorted item: its run (tile base + ballot ranks), the run's key from the head,
//                            and the supporters' counts, sums, minima and maxima by a segmented scan across the wave
//                            (a head starts a segment): the last lane of every segment folds it into the run's figures
//                            with integer atomics.  A run costs one set of atomics per wave it spans: a run of one
//                            candidate one set, a run of a hundred thousand about 1600, spread over as many waves.
//  kc_link_emit_kernel       a thread per run = per directed record: the 48-byte record as three 16-byte stores, and the
//                            link statistics (an undirected link is counted at its from < to record).
//  kc_link_end_first_kernel  a thread per end: the first run whose `from` is not below it, by binary search.
//
// No workgroup waits for another; every loop's trip count comes from the input (a read's slots, the scan's log steps,
// the search's).  All figures are integers, so the result does not depend on the order in which the atomics arrive.
#pragma once
#include "kc_depth.hpp"

namespace kc {

constexpr int LINK_TILE = 256;  // sorted items a workgroup: a thread each
constexpr int LINK_SCAN_ITEMS = 4;  // consecutive counts a thread of the tile scan holds
constexpr int LINK_SCAN_SHIFT = 10;
constexpr uint64_t LINK_SCAN_TILE = 1ull << LINK_SCAN_SHIFT;
static_assert(LINK_SCAN_TILE == (uint64_t)LINK_TILE * LINK_SCAN_ITEMS, "a workgroup scans a tile");
constexpr uint32_t LINK_NO_END = 0xFFFFFFFFu;
constexpr uint32_t LINK_MAX_SLACK = 1024, LINK_MAX_OVERLAP = 65535, LINK_MAX_READ_ALNS = 64;
constexpr uint32_t LINK_GAP_BIAS = 65536;  // a gap lies in (-65536, 65536): biased it fits under the kind at bit 24
constexpr uint32_t LINK_SPAN = 1u << 24;

enum { LKS_NONE = 0, LKS_FILTERED, LKS_PASSED, LKS_OVER_CAP, LKS_SPLINT_CANDS, LKS_GAP_OUT, LKS_SPAN_CANDS, LKS_TOO_FAR, LKS_LINKS,
       LKS_SPLINT_ONLY, LKS_SPAN_ONLY, LKS_BOTH, LKS_ENDS, LKS_SLOT_TOTAL, LKS_CAND_TOTAL, LKS_RUN_TOTAL, LKS_SORT_TOTAL, LKS_COUNT };

struct LinkArgs {
  const uint32_t *offs;  // the index's n_ctgs + 1 starts
  uint32_t n_ctgs;
  const uint4 *alns;  // kc_gap_aln
  uint64_t n_alns;
  const uint64_t *offsets;  // the reads'
  uint64_t nreads;
  const uint4 *pairs;  // kc_pair_rec or null
  uint32_t min_score, min_len, end_slack, max_overlap, max_splint_gap, insert_avg, max_insert, max_read_alns;
  uint64_t *st;
  uint64_t *rfirst;  // [nreads] the reads' passing records, then their first slots within their tile
  uint64_t *rbase;   // [tiles of reads] the tiles' first slots
  uint32_t *rcur;    // [nreads] cursors of the fill pass: the reads' passing records when it is done
  uint4 *info;       // [slots]
  uint64_t *ufirst;  // [nreads + npairs] a thread's candidates, then its first within its tile
  uint64_t *ubase;   // [tiles of threads] the tiles' first candidates
  uint64_t *keys;    // [2 * candidates]
  uint32_t *payload;  // [candidates]
};

// the figures of a run, or of a part of one
struct LinkSeg {
  uint64_t cnt;  // splints | spans << 32
  int64_t ssum, psum;
  int32_t smin, smax, pmin, pmax;
  __device__ __forceinline__ LinkSeg join(const LinkSeg &y) const {
    return LinkSeg{cnt + y.cnt,           ssum + y.ssum,
                   psum + y.psum,         smin < y.smin ? smin : y.smin,
                   smax > y.smax ? smax : y.smax, pmin < y.pmin ? pmin : y.pmin,
                   pmax > y.pmax ? pmax : y.pmax};
  }
  __device__ __forceinline__ LinkSeg up(int o) const {
    return LinkSeg{__shfl_up(cnt, o),  __shfl_up(ssum, o), __shfl_up(psum, o), __shfl_up(smin, o),
                   __shfl_up(smax, o), __shfl_up(pmin, o), __shfl_up(pmax, o)};
  }
};
constexpr int32_t LINK_MIN_INIT = 0x7F7F7F7F, LINK_MAX_INIT = (int32_t)0x80808080u;  // what a memset gives

struct LinkAcc {
  uint64_t *key;        // [runs] from << 32 | to
  uint64_t *cnt;        // [runs] zeroed
  uint64_t *ssum, *psum;  // [runs] zeroed, two's complement
  int32_t *smin, *pmin;   // [runs] LINK_MIN_INIT
  int32_t *smax, *pmax;   // [runs] LINK_MAX_INIT
};

constexpr int LINK_STAT_TPB = 1024;  // threads a workgroup of the kernels that count statistics (wg_stats, kc_kit.hpp)

template <bool WRITE>
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_link_group_kernel(LinkArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int cls = -1;
  if (i < a.n_alns) {
    const DepthRec r = depth_load(a.alns, i);
    if (r.kind == GAP_KIND_NONE)
      cls = LKS_NONE;
    else if (r.score < a.min_score || r.cstop - r.cstart < a.min_len)
      cls = LKS_FILTERED;
    else {
      cls = LKS_PASSED;
      if (!WRITE)
        atomicAdd((unsigned long long *)&a.rfirst[r.read], 1ull);
      else {
        const uint64_t slot = a.rbase[r.read >> LINK_SCAN_SHIFT] + a.rfirst[r.read] + (uint64_t)atomicAdd(&a.rcur[r.read], 1u);
        const uint32_t L = (uint32_t)(a.offsets[r.read + 1] - a.offsets[r.read]);  // rstop <= L <= 1024: checked
        const uint32_t len = a.offs[r.ctg + 1] - 1u - a.offs[r.ctg];
        const uint32_t qs = r.orient ? L - r.rstop : r.rstart, qe = r.orient ? L - r.rstart : r.rstop;
        const uint32_t e_right = len - r.cstop, e_left = r.cstart;
        const uint32_t e_leave = r.orient ? e_left : e_right, e_enter = r.orient ? e_right : e_left;
        a.info[slot] = make_uint4(qs | (qe << 16), (r.ctg << 1) | r.orient, e_leave <= a.end_slack ? e_leave : LINK_NO_END,
                                  e_enter <= a.end_slack ? e_enter : LINK_NO_END);
      }
    }
  }
  if (!WRITE) {
    const int k[3] = {LKS_NONE, LKS_FILTERED, LKS_PASSED};
    const uint32_t mine[3] = {cls == LKS_NONE ? 1u : 0u, cls == LKS_FILTERED ? 1u : 0u, cls == LKS_PASSED ? 1u : 0u};
    wg_stats<3>(a.st, k, mine);
  }
}

// candidate c of the call: both directions' keys as one 16-byte store, and the payload
__device__ __forceinline__ void link_put(const LinkArgs &a, uint64_t c, uint32_t from, uint32_t to, uint32_t kind, int64_t gap) {
  ulonglong2 k;
  k.x = ((uint64_t)from << 32) | to;
  k.y = ((uint64_t)to << 32) | from;
  *(ulonglong2 *)(a.keys + 2 * c) = k;
  a.payload[c] = kind | (uint32_t)(gap + (int64_t)LINK_GAP_BIAS);
}

template <bool WRITE>
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_link_cands_kernel(LinkArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t npairs = a.pairs ? a.nreads >> 1 : 0, units = a.nreads + npairs;
  uint32_t n = 0, n_span = 0, gap_out = 0, over = 0, too_far = 0;
  const uint64_t at = (WRITE && t < units) ? a.ubase[t >> LINK_SCAN_SHIFT] + a.ufirst[t] : 0;
  if (t < a.nreads) {
    const uint64_t f = a.rbase[t >> LINK_SCAN_SHIFT] + a.rfirst[t], c = a.rcur[t];
    if (c > (uint64_t)a.max_read_alns)
      over = 1;
    else {
      for (uint64_t i = 0; i < c; i++) {
        const uint4 x = a.info[f + i];
        if (x.z == LINK_NO_END) continue;  // it does not leave
        const int64_t qs_a = x.x & 0xFFFFu, qe_a = x.x >> 16;
        for (uint64_t j = 0; j < c; j++) {
          const uint4 y = a.info[f + j];
          const int64_t qs_b = y.x & 0xFFFFu, qe_b = y.x >> 16;
          if ((x.y >> 1) == (y.y >> 1) || y.w == LINK_NO_END || !(qs_a < qs_b && qe_a < qe_b)) continue;
          const int64_t gap = (qs_b - qe_a) - (int64_t)x.z - (int64_t)y.w;
          if (gap < -(int64_t)a.max_overlap || gap > (int64_t)a.max_splint_gap) {
            gap_out++;
            continue;
          }
          // a leaves through its right end iff orient 0; b enters through its left end iff orient 0
          if (WRITE) link_put(a, at + n, x.y ^ 1u, y.y, 0u, gap);
          n++;
        }
      }
    }
  } else if (t < units) {
    const uint64_t p = t - a.nreads;
    const uint4 pr = a.pairs[p];
    if (pr.x != LINK_NO_END && pr.y != LINK_NO_END) {
      const DepthRec b0 = depth_load(a.alns, pr.x), b1 = depth_load(a.alns, pr.y);
      if (b0.ctg != b1.ctg) {
        int64_t d[2];
        uint32_t end[2];
#pragma unroll
        for (int s = 0; s < 2; s++) {
          const DepthRec &b = s ? b1 : b0;
          const int64_t L = (int64_t)(a.offsets[2 * p + s + 1] - a.offsets[2 * p + s]);
          const int64_t len = (int64_t)(a.offs[b.ctg + 1] - 1u - a.offs[b.ctg]);
          d[s] = b.orient ? (int64_t)b.cstop + (L - (int64_t)b.rstop) : len - ((int64_t)b.cstart - (int64_t)b.rstart);
          end[s] = (b.ctg << 1) | (b.orient ? 0u : 1u);
        }
        if (d[0] + d[1] > (int64_t)a.max_insert)
          too_far = 1;
        else {
          if (WRITE) link_put(a, at, end[0], end[1], LINK_SPAN, (int64_t)a.insert_avg - d[0] - d[1]);
          n = n_span = 1;
        }
      }
    }
  }
  if (!WRITE) {
    if (t < units) a.ufirst[t] = n;
    const int k[5] = {LKS_SPLINT_CANDS, LKS_GAP_OUT, LKS_OVER_CAP, LKS_SPAN_CANDS, LKS_TOO_FAR};
    const uint32_t mine[5] = {n - n_span, gap_out, over, n_span, too_far};
    wg_stats<5>(a.st, k, mine);
  }
}

// exclusive scan of every tile of LINK_SCAN_TILE counts of v[0, n) in place; tile_sums[tile] = the tile's total
__global__ void __launch_bounds__(LINK_TILE) kc_link_tile_scan_kernel(uint64_t *v, uint64_t n, uint64_t *tile_sums) {
  __shared__ uint64_t ws[LINK_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * LINK_SCAN_TILE + (uint64_t)tid * LINK_SCAN_ITEMS;
  uint64_t x[LINK_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < LINK_SCAN_ITEMS; k++) {
    x[k] = first + k < n ? v[first + k] : 0ull;
    s += x[k];
  }
  uint64_t inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(inc, o);
    inc += lane >= o ? t : 0ull;
  }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  uint64_t p = inc - s;
  for (int w = 0; w < wv; w++) p += ws[w];
#pragma unroll
  for (int k = 0; k < LINK_SCAN_ITEMS; k++) {
    if (first + k < n) v[first + k] = p;
    p += x[k];
  }
  if (tid == LINK_TILE - 1) tile_sums[blockIdx.x] = p;
}

// the thread's item is the first of its run
__device__ __forceinline__ bool link_head(const uint64_t *keys, uint64_t i, uint64_t n) { return i < n && (i == 0 || keys[i] != keys[i - 1]); }

__global__ void __launch_bounds__(LINK_TILE) kc_link_heads_kernel(const uint64_t *keys, uint64_t n, uint64_t *tile_heads) {
  __shared__ uint32_t ws[LINK_TILE / 64];
  const int tid = threadIdx.x;
  const uint32_t c = wave_count(link_head(keys, (uint64_t)blockIdx.x * LINK_TILE + tid, n));
  if ((tid & 63) == 0) ws[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) tile_heads[blockIdx.x] = (uint64_t)(ws[0] + ws[1] + ws[2] + ws[3]);
}
static_assert(LINK_TILE == 256, "four waves a workgroup");

// keys, perm: the sorted items and where they came from (item 2c and 2c + 1 are candidate c); tile_first: the scanned heads
__global__ void __launch_bounds__(LINK_TILE) kc_link_reduce_kernel(const uint64_t *keys, const uint32_t *perm, const uint32_t *payload,
                                                                    uint64_t n, const uint64_t *tile_first, LinkAcc acc) {
  __shared__ uint32_t ws[LINK_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * LINK_TILE + tid;
  const bool valid = i < n, head = link_head(keys, i, n);
  const unsigned long long heads = __ballot(head), live = __ballot(valid);
  if (lane == 0) ws[wv] = (uint32_t)__popcll(heads);
  __syncthreads();
  uint64_t run = tile_first[blockIdx.x] + (uint64_t)__popcll(heads & ((2ull << lane) - 1ull));  // one past the item's run
  for (int w = 0; w < wv; w++) run += ws[w];
  run -= 1;  // the first item of all is a head: never below 0 for a valid item
  LinkSeg s{0ull, 0, 0, LINK_MIN_INIT, LINK_MAX_INIT, LINK_MIN_INIT, LINK_MAX_INIT};
  if (valid) {
    if (head) acc.key[run] = keys[i];
    const uint32_t pl = payload[perm[i] >> 1];
    const int32_t gap = (int32_t)(pl & (LINK_SPAN - 1u)) - (int32_t)LINK_GAP_BIAS;
    if (pl & LINK_SPAN)
      s = LinkSeg{1ull << 32, 0, gap, LINK_MIN_INIT, LINK_MAX_INIT, gap, gap};
    else
      s = LinkSeg{1ull, gap, 0, gap, gap, LINK_MIN_INIT, LINK_MAX_INIT};
  }
  // segmented inclusive scan: a head starts a segment, and so does lane 0 (its run may have begun in another wave) and
  // every lane past the end
  wave_seg_scan(s, head || lane == 0 || !valid, lane);
  const bool next_live = lane < 63 && ((live >> (lane + 1)) & 1ull), next_head = lane < 63 && ((heads >> (lane + 1)) & 1ull);
  if (valid && (!next_live || next_head)) {  // the last lane of its segment
    atomicAdd((unsigned long long *)&acc.cnt[run], (unsigned long long)s.cnt);
    if ((uint32_t)s.cnt) {
      if (s.ssum) atomicAdd((unsigned long long *)&acc.ssum[run], (unsigned long long)s.ssum);
      atomicMin(&acc.smin[run], s.smin);
      atomicMax(&acc.smax[run], s.smax);
    }
    if (s.cnt >> 32) {
      if (s.psum) atomicAdd((unsigned long long *)&acc.psum[run], (unsigned long long)s.psum);
      atomicMin(&acc.pmin[run], s.pmin);
      atomicMax(&acc.pmax[run], s.pmax);
    }
  }
}

// kc_ctg_link: {u32 from, to, splints, spans; i32 splint_gap_min, splint_gap_max, span_gap_min, span_gap_max; i64 splint_gap_sum,
// span_gap_sum}.  out == nullptr: the statistics only (a size query).
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_link_emit_kernel(LinkAcc acc, uint64_t n_runs, uint4 *out, uint64_t *st) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int cls = -1;
  bool first = false;
  if (j < n_runs) {
    const uint64_t key = acc.key[j], cnt = acc.cnt[j];
    const uint32_t from = (uint32_t)(key >> 32), to = (uint32_t)key, splints = (uint32_t)cnt, spans = (uint32_t)(cnt >> 32);
    first = j == 0 || (uint32_t)(acc.key[j - 1] >> 32) != from;
    if (from < to) cls = splints && spans ? LKS_BOTH : splints ? LKS_SPLINT_ONLY : LKS_SPAN_ONLY;
    if (out) {
      const uint64_t ssum = splints ? acc.ssum[j] : 0ull, psum = spans ? acc.psum[j] : 0ull;
      out[3 * j] = make_uint4(from, to, splints, spans);
      out[3 * j + 1] = make_uint4(splints ? (uint32_t)acc.smin[j] : 0u, splints ? (uint32_t)acc.smax[j] : 0u, spans ? (uint32_t)acc.pmin[j] : 0u,
                                  spans ? (uint32_t)acc.pmax[j] : 0u);
      out[3 * j + 2] = make_uint4((uint32_t)ssum, (uint32_t)(ssum >> 32), (uint32_t)psum, (uint32_t)(psum >> 32));
    }
  }
  const int k[5] = {LKS_LINKS, LKS_SPLINT_ONLY, LKS_SPAN_ONLY, LKS_BOTH, LKS_ENDS};
  const uint32_t mine[5] = {cls >= 0 ? 1u : 0u, cls == LKS_SPLINT_ONLY ? 1u : 0u, cls == LKS_SPAN_ONLY ? 1u : 0u, cls == LKS_BOTH ? 1u : 0u,
                            first ? 1u : 0u};
  wg_stats<5>(st, k, mine);
}

// end_first[e], e in [0, n_ends]: the first run whose `from` is at least e; n_runs for e = n_ends
__global__ void kc_link_end_first_kernel(const uint64_t *run_key, uint64_t n_runs, uint64_t n_ends, uint64_t *end_first) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > n_ends) return;
  uint64_t lo = 0, hi = n_runs;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((run_key[mid] >> 32) < e)
      lo = mid + 1;
    else
      hi = mid;
  }
  end_first[e] = lo;
}

}  // namespace kc
