// kc_scaffold.hpp -- the walk over the contig links (kc_scaffold): one partner per contig end, claimed overlaps checked
// against the contigs' text, the chosen edges walked by pointer jumping, and the scaffolds written as a new seq block --
// the second half of scaffolding, behind kc_links.hpp.  The reference holds no code for it (no cgraph, no scaffolding in
// src/), so the rules are this project's own definition (pinned statement by statement by
// tests/scaffold_model.py); no parity with MetaHipMer is claimed.  include/kcount_mi355.h states the rules in full.
//
// End 2u is the left end of contig u, 2u + 1 its right end.  An oriented node is v = 2u + s (s = 1: the reverse
// complement); v is ENTERED through end v and LEFT through end v ^ 1, so next(v) = the partner of end v ^ 1, as a node
// number, and the edge a node is entered through is filed under the node's own number.
//
// Kernels, in the order of the call (kc_link_end_first_kernel, the three kc_unitig_*_jump / cut kernels and
// kc_scan_kernel<1> / <2> are called as they stand):
//  kc_scaf_check_kernel    a thread per record: the record's own rules, its predecessor's key, and its mirror by a binary
//                          search over the records; the lowest bad index by a 64-bit atomic minimum.  Writes the keys
//                          from << 32 | to that kc_link_end_first_kernel searches.
//  kc_scaf_choose_kernel   a WAVE per end: the lanes stride over the end's row and keep (best, second's support), six
//                          butterfly steps merge them.  A wave, not a thread, because a row's length is unbounded (a hub
//                          end has thousands of partners, each three dependent 16-byte loads for one thread), while the
//                          ends are two a contig: the idle lanes of a short row cost nothing that shows.
//  kc_scaf_edge_kernel     a wave per end; the wave of the smaller end of a chosen edge verifies it and writes both
//                          ends' {partner, join}, every other wave of an end without edge writes {none}: every entry is
//                          written exactly once.  An overlap is compared 64 bytes a trip (coalesced byte loads, one
//                          ballot), B read forwards and A from its tail, either through the reverse complement where the
//                          node says so.
//  kc_scaf_next_kernel     a thread per contig: next[] of its two nodes and the first buffer of the cycle search.
//  kc_scaf_weight_kernel   a thread per contig, behind the cut: the first buffer of the second ranking, whose weight is
//                          len(pred) + join -- the distance between the starts of two neighbours' texts -- and the
//                          call's byte total in 64 bits, so that 2^31 bytes are refused before a 32-bit sum can wrap.
//  kc_scaf_select_kernel   a thread per node; the tail of a path knows members, bytes and head: the path whose head is
//                          the smaller contig is the one emitted.
//  kc_scaf_members_kernel  a thread per node of an emitted path: its member record, its segment's start in the block,
//                          its contig's member index, its scaffold's N and overlap bases (32-bit integer atomics).
//  kc_scaf_records_kernel  a thread per contig: a head writes its scaffold's 32-byte record.
//  kc_scaf_write_kernel    a thread per ALIGNED 16 bytes of the block: a binary search over the segments' starts finds its
//                          first member, then it walks on over as many members as its bytes span -- N runs, text
//                          forwards or reverse-complemented from the far end, separators -- and stores 16 bytes at once;
//                          the block's first and last partial chunk are byte stores.  Plain vector stores only.
//
// No workgroup waits for another; every loop's trip count comes from the input (a row, the slack range, an overlap's
// length, a search's steps, the members a chunk spans); the jump rounds are launches the host counts.  All figures are
// integers, so the result does not depend on the order in which the atomics arrive.
#pragma once
#include "kc_links.hpp"
#include "kc_unitig.hpp"

namespace kc {

constexpr int SCAF_TPB = 256;
constexpr uint32_t SCAF_NONE = 0xFFFFFFFFu;
constexpr uint32_t SCAF_MAX_SLACK = 64;
constexpr uint32_t SCAF_CIRCULAR = 1;

// device statistics of a call (uint64_t each); the cut kernel counts the cycles at UST_CIRCULAR
enum { SCS_CIRCULAR = 0, SCS_BAD, SCS_QUALIFYING, SCS_ENDS_BEST, SCS_AMBIGUOUS, SCS_NOT_MUTUAL, SCS_CHOSEN, SCS_OV_CHECKED, SCS_OV_REJECTED,
       SCS_JOINED, SCS_SINGLE, SCS_LONGEST, SCS_N2, SCS_OV2, SCS_BYTES2, SCS_TAILS, SCS_TOTALS, SCS_MTOTAL = SCS_TOTALS + 2, SCS_COUNT };
static_assert(SCS_CIRCULAR == UST_CIRCULAR, "kc_unitig_cut_kernel counts there");

__device__ __forceinline__ bool scaf_kind_ok(uint32_t c, int32_t lo, int32_t hi, int64_t sum) {
  if (c == 0) return lo == 0 && hi == 0 && sum == 0;
  if (!(lo >= -(int32_t)LINK_MAX_OVERLAP && lo <= hi && hi <= 65535)) return false;
  return (int64_t)c * lo <= sum && sum <= (int64_t)c * hi;
}

__device__ __forceinline__ uint64_t scaf_key(const uint4 &a) { return ((uint64_t)a.x << 32) | a.y; }

// links: kc_ctg_link as three uint4 {from, to, splints, spans} {the four minima and maxima} {the two sums}
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_check_kernel(const uint4 *links, uint64_t n_links, uint64_t n_ends, uint64_t *keys,
                                                                 uint64_t *st) {
  const uint64_t i = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  if (i >= n_links) return;
  const uint4 a = links[3 * i], b = links[3 * i + 1], s = links[3 * i + 2];
  const uint64_t key = scaf_key(a);
  keys[i] = key;
  bool ok = a.x < n_ends && a.y < n_ends && (a.x >> 1) != (a.y >> 1) && (uint64_t)a.z + a.w >= 1;
  ok = ok && scaf_kind_ok(a.z, (int32_t)b.x, (int32_t)b.y, (int64_t)(s.x | ((uint64_t)s.y << 32)));
  ok = ok && scaf_kind_ok(a.w, (int32_t)b.z, (int32_t)b.w, (int64_t)(s.z | ((uint64_t)s.w << 32)));
  if (ok && i) ok = key > scaf_key(links[3 * (i - 1)]);
  if (ok) {  // the mirror: the first record whose key is not below (to, from)
    const uint64_t want = ((uint64_t)a.y << 32) | a.x;
    uint64_t lo = 0, hi = n_links;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (scaf_key(links[3 * mid]) < want)
        lo = mid + 1;
      else
        hi = mid;
    }
    ok = lo < n_links;
    if (ok) {
      const uint4 ma = links[3 * lo], mb = links[3 * lo + 1], ms = links[3 * lo + 2];
      ok = scaf_key(ma) == want && ma.z == a.z && ma.w == a.w && mb.x == b.x && mb.y == b.y && mb.z == b.z && mb.w == b.w && ms.x == s.x &&
           ms.y == s.y && ms.z == s.z && ms.w == s.w;
    }
  }
  if (!ok) atomicMin((unsigned long long *)&st[SCS_BAD], (unsigned long long)i);
}

// floor((2 sum + c) / (2 c)): the mean, rounded half up
__device__ __forceinline__ int64_t scaf_floor_mean(int64_t sum, int64_t c) {
  const int64_t a = 2 * sum + c, b = 2 * c;
  int64_t q = a / b;
  if (a % b != 0 && a < 0) q--;
  return q;
}

// An end's best record so far and the support of its second.  The order: (support, splints, smaller `to`) as (hi, lo); a
// qualifying record's support is at least 1, so hi = 0 is none.
struct ScafBest {
  uint64_t hi, lo, idx, second;
  __device__ __forceinline__ ScafBest join(const ScafBest &y) const {
    if (y.hi > hi || (y.hi == hi && y.lo > lo)) return ScafBest{y.hi, y.lo, y.idx, y.second > hi ? y.second : hi};
    return ScafBest{hi, lo, idx, y.hi > second ? y.hi : second};
  }
  __device__ __forceinline__ ScafBest across(int o) const {
    return ScafBest{__shfl_xor(hi, o), __shfl_xor(lo, o), __shfl_xor(idx, o), __shfl_xor(second, o)};
  }
};

// pick[e] = {best(e).to or SCAF_NONE, its gap, e is ambiguous, 0}
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_choose_kernel(const uint4 *links, const uint64_t *end_first, uint64_t n_ends,
                                                                  uint32_t min_splints, uint32_t min_spans, uint32_t permille, uint4 *pick,
                                                                  uint64_t *st) {
  const int lane = threadIdx.x & 63;
  const uint64_t e = (uint64_t)blockIdx.x * (SCAF_TPB / 64) + (threadIdx.x >> 6);
  if (e >= n_ends) return;  // the whole wave
  const uint64_t first = end_first[e], last = end_first[e + 1];
  ScafBest b{0, 0, 0, 0};
  uint32_t q = 0;
  for (uint64_t r = first + lane; r < last; r += 64) {
    const uint4 a = links[3 * r];
    if (a.z < min_splints && a.w < min_spans) continue;
    q++;
    b = b.join(ScafBest{(uint64_t)a.z + a.w, ((uint64_t)a.z << 32) | (uint32_t)~a.y, r, 0});
  }
  b = wave_join(b);
  wave_add(st, SCS_QUALIFYING, q);
  if (lane) return;
  const uint64_t bhi = b.hi, bidx = b.idx, second = b.second;
  uint4 out = make_uint4(SCAF_NONE, 0u, 0u, 0u);
  if (bhi) {
    const uint4 a = links[3 * bidx], s = links[3 * bidx + 2];
    const int64_t gap = a.z ? scaf_floor_mean((int64_t)(s.x | ((uint64_t)s.y << 32)), (int64_t)a.z)
                            : scaf_floor_mean((int64_t)(s.z | ((uint64_t)s.w << 32)), (int64_t)a.w);
    const bool amb = second && second * 1000ull > bhi * (uint64_t)permille;
    out = make_uint4(a.y, (uint32_t)(int32_t)gap, amb ? 1u : 0u, 0u);
    atomicAdd((unsigned long long *)&st[SCS_ENDS_BEST], 1ull);
    if (amb) atomicAdd((unsigned long long *)&st[SCS_AMBIGUOUS], 1ull);
  }
  pick[e] = out;
}

// byte j of a node's text: the contig at src[0, len), as it stands or reverse-complemented
__device__ __forceinline__ uint32_t scaf_text(const uint8_t *src, uint32_t len, bool rev, uint32_t j) {
  return rev ? base_comp(src[len - 1u - j]) : (uint32_t)src[j];
}

// link[e] = {the partner of end e or SCAF_NONE, the join}
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_edge_kernel(const uint4 *pick, uint64_t n_ends, const uint8_t *seqs, const uint32_t *offs,
                                                                uint32_t slack, uint2 *link, uint64_t *st) {
  const int lane = threadIdx.x & 63;
  const uint64_t e = (uint64_t)blockIdx.x * (SCAF_TPB / 64) + (threadIdx.x >> 6);
  if (e >= n_ends) return;
  const uint4 p = pick[e];
  bool mutual = false, chosen = false;
  if (p.x != SCAF_NONE) {
    const uint4 o = pick[p.x];
    mutual = o.x == (uint32_t)e;
    chosen = mutual && !p.z && !o.z;
  }
  if (!chosen) {
    if (lane == 0) {
      link[e] = make_uint2(SCAF_NONE, 0u);
      if (p.x != SCAF_NONE && !mutual) atomicAdd((unsigned long long *)&st[SCS_NOT_MUTUAL], 1ull);
    }
    return;
  }
  const uint32_t f = p.x;
  if (f < e) return;  // the smaller end's wave writes both
  const int32_t gap = (int32_t)p.y;
  int32_t join = gap;
  bool found = true;
  if (gap < 0) {
    // A: the node left through e, e ^ 1 (reversed iff e is even); B: the node entered through f (reversed iff f is odd)
    const uint32_t ua = (uint32_t)(e >> 1), ub = f >> 1;
    const uint32_t la = offs[ua + 1] - 1u - offs[ua], lb = offs[ub + 1] - 1u - offs[ub];
    const uint8_t *sa = seqs + offs[ua], *sb = seqs + offs[ub];
    const bool ra = !(e & 1), rb = f & 1u;
    const int64_t o = -(int64_t)gap, lim = la < lb ? la : lb;
    found = false;
    for (uint32_t k = 0; k <= 2u * slack && !found; k++) {
      const int64_t d = (k + 1u) >> 1, cand = (k & 1u) ? o + d : o - d;
      if (cand < 1 || cand >= lim) continue;
      const uint32_t t = (uint32_t)cand;
      bool same = true;
      for (uint32_t i0 = 0; i0 < t && same; i0 += 64) {
        const uint32_t i = i0 + lane;
        bool ok = true;
        if (i < t) {
          const uint32_t cb = scaf_text(sb, lb, rb, i);
          ok = ai_is_acgt_upper(cb) && scaf_text(sa, la, ra, la - t + i) == cb;
        }
        same = __ballot(!ok) == 0ull;
      }
      if (same) {
        found = true;
        join = -(int32_t)t;
      }
    }
  }
  if (lane) return;
  link[e] = found ? make_uint2(f, (uint32_t)join) : make_uint2(SCAF_NONE, 0u);
  link[f] = found ? make_uint2((uint32_t)e, (uint32_t)join) : make_uint2(SCAF_NONE, 0u);
  atomicAdd((unsigned long long *)&st[SCS_CHOSEN], 1ull);
  if (gap < 0) atomicAdd((unsigned long long *)&st[SCS_OV_CHECKED], 1ull);
  atomicAdd((unsigned long long *)&st[found ? SCS_JOINED : SCS_OV_REJECTED], 1ull);
}

// next2[u] = {next(u,+), next(u,-)}: the partners of ends 2u + 1 and 2u; cyc4[u] = {next(u,+), u, next(u,-), u}
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_next_kernel(const uint2 *link, uint32_t n, uint2 *next2, uint4 *cyc4) {
  const uint64_t u = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  if (u >= n) return;
  const uint32_t n0 = link[2 * u + 1].x, n1 = link[2 * u].x;
  next2[u] = make_uint2(n0, n1);
  cyc4[u] = make_uint4(n0, (uint32_t)u, n1, (uint32_t)u);
}

// rank4: what kc_unitig_cut_kernel wrote, {pred(u,+) or itself, 1 or 0, pred(u,-) or itself, 1 or 0}; next2: behind the cut.
// pos4[u]: the same predecessors with the weight len(pred) + join, the distance from the start of the predecessor's text
// to the start of the node's (its virtual start where an overlap is merged away: at least 1, an overlap is shorter than
// either text).
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_weight_kernel(const uint4 *rank4, const uint2 *next2, const uint2 *link, const uint32_t *offs,
                                                                  uint32_t n, uint4 *pos4, uint64_t *st) {
  const uint64_t u = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  unsigned long long nb = 0, ob = 0, bytes = 0, tails = 0;
  if (u < n) {
    const uint4 r = rank4[u];
    const uint2 nx = next2[u];
    const uint32_t len = offs[u + 1] - 1u - offs[u];
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const uint32_t pred = s ? r.z : r.x, has = s ? r.w : r.y;
      if (has) {
        const int32_t j = (int32_t)link[2 * u + s].y;
        w[s] = offs[(pred >> 1) + 1] - 1u - offs[pred >> 1] + (uint32_t)j;
        nb += j > 0 ? (unsigned long long)j : 0ull;
        ob += j < 0 ? (unsigned long long)-(int64_t)j : 0ull;
      }
      bytes += w[s];
      if ((s ? nx.y : nx.x) == SCAF_NONE) {
        bytes += len;
        tails++;
      }
    }
    pos4[u] = make_uint4(r.x, w[0], r.z, w[1]);
  }
  wave_add(st, SCS_N2, nb);
  wave_add(st, SCS_OV2, ob);
  wave_add(st, SCS_BYTES2, bytes);
  wave_add(st, SCS_TAILS, tails);
}

// rank, pos: {head, members before} and {head, text start} of every node; cyc: the cycle search's last buffer.  size, num,
// mcnt, info: zeroed, one entry a contig; info = {members, bases, flags, 1 + the head's strand}.
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_select_kernel(const uint2 *rank, const uint2 *pos, const uint2 *cyc, const uint32_t *next,
                                                                  const uint32_t *offs, uint32_t nn, uint64_t *size, uint64_t *num, uint64_t *mcnt,
                                                                  uint4 *info, uint64_t *st) {
  const uint64_t g = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  const uint32_t v = (uint32_t)g;
  unsigned long long single = 0, longest = 0;
  if (g < nn && next[v] == SCAF_NONE) {  // a tail
    const uint2 e = rank[v];
    const uint32_t h = e.x;
    if ((h >> 1) < (v >> 1) || (h == v && !(v & 1u))) {
      const uint32_t bases = pos[v].y + (offs[(v >> 1) + 1] - 1u - offs[v >> 1]);
      size[h >> 1] = (uint64_t)bases + 1u;
      num[h >> 1] = 1;
      mcnt[h >> 1] = (uint64_t)e.y + 1u;
      info[h >> 1] = make_uint4(e.y + 1u, bases, cyc[h].x != SCAF_NONE ? SCAF_CIRCULAR : 0u, 1u + (h & 1u));
      single = e.y == 0u;
      longest = bases;
    }
  }
  wave_add(st, SCS_SINGLE, single);
  longest = wave_max(longest);
  if ((threadIdx.x & 63) == 0 && longest) atomicMax((unsigned long long *)&st[SCS_LONGEST], longest);
}

// off, snum, mfirst: size, num and mcnt after their scans.  members: kc_scaf_member as a uint4 {ctg, join, out_pos, orient};
// seg[i]: the block position where member i's segment -- its N run, then its text -- starts; seg[n] = total.
// acc: zeroed, {N bases, overlap bases} a scaffold.  offsets, ctg_member: may be null.
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_members_kernel(const uint2 *rank, const uint2 *pos, const uint2 *link, const uint4 *info,
                                                                   const uint64_t *off, const uint64_t *snum, const uint64_t *mfirst, uint32_t nn,
                                                                   uint32_t total, uint64_t n_scaf, uint4 *members, uint32_t *seg, uint32_t *acc,
                                                                   uint64_t *offsets, uint32_t *ctg_member) {
  const uint64_t g = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  if (g >= nn) return;
  const uint32_t v = (uint32_t)g;
  if (v == 0) {
    seg[nn >> 1] = total;
    if (offsets) offsets[n_scaf] = total;
  }
  const uint2 e = rank[v];
  const uint32_t hi = e.x >> 1;
  if (info[hi].w != 1u + (e.x & 1u)) return;  // the twin of an emitted path
  const uint32_t at = (uint32_t)off[hi], idx = (uint32_t)mfirst[hi] + e.y;
  const uint64_t s = snum[hi];
  const int32_t j = e.y ? (int32_t)link[v].y : 0;
  const uint32_t start = at + pos[v].y;  // of the node's whole text
  members[idx] = make_uint4(v >> 1, (uint32_t)j, j < 0 ? start + (uint32_t)-j : start, v & 1u);
  seg[idx] = start - (uint32_t)j;
  if (ctg_member) ctg_member[v >> 1] = idx;
  if (e.y == 0u && offsets) offsets[s] = at;
  if (j > 0) atomicAdd(&acc[2 * s], (uint32_t)j);
  if (j < 0) atomicAdd(&acc[2 * s + 1], (uint32_t)-j);
}

// kc_scaffold_rec as two uint4: {first_member, n_members, len, n_bases} {overlap_bases, flags, 0, 0}
__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_records_kernel(const uint4 *info, const uint64_t *snum, const uint64_t *mfirst,
                                                                   const uint32_t *acc, uint32_t n, uint4 *scaffolds) {
  const uint64_t u = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  if (u >= n) return;
  const uint4 f = info[u];
  if (!f.w) return;
  const uint64_t s = snum[u];
  scaffolds[2 * s] = make_uint4((uint32_t)mfirst[u], f.x, f.y, acc[2 * s]);
  scaffolds[2 * s + 1] = make_uint4(acc[2 * s + 1], f.z, 0u, 0u);
}

// the member a writer thread is in
struct ScafSeg {
  uint32_t s1;  // where the next segment starts
  uint32_t s0, nrun, skip, len, base, fill;
  bool rev;
};
// FILL: fill[i] is where the bytes of member i's run lie in the fill buffer, SCAF_NONE for a run of N (kc_close.hpp)
template <bool FILL>
__device__ __forceinline__ ScafSeg scaf_seg_load(const uint4 *members, const uint32_t *seg, const uint32_t *fill, const uint32_t *offs, uint32_t i) {
  const uint4 m = members[i];
  const int32_t j = (int32_t)m.y;
  const uint32_t base = offs[m.x];
  return ScafSeg{seg[i + 1], seg[i], j > 0 ? (uint32_t)j : 0u, j < 0 ? (uint32_t)-j : 0u, offs[m.x + 1] - 1u - base, base,
                 FILL ? fill[i] : SCAF_NONE, m.w != 0u};
}

// The body of kc_scaf_write_kernel and kc_close_write_kernel.  Thread t owns out[16 t - mis, 16 t - mis + 16) cut to
// [0, total): mis = out's address & 15, so every whole chunk is an aligned 16-byte store.  n members, seg[0] = 0,
// seg[n] = total, seg ascending.
template <bool FILL>
__device__ __forceinline__ void scaf_write_body(const uint4 *members, const uint32_t *seg, const uint32_t *fill, uint32_t n, const uint8_t *src,
                                                const uint32_t *offs, const uint8_t *buf, uint32_t mis, uint32_t total, uint8_t *out) {
  const uint64_t t = (uint64_t)blockIdx.x * SCAF_TPB + threadIdx.x;
  const int64_t p0 = (int64_t)t * 16 - (int64_t)mis;
  if (p0 >= (int64_t)total) return;
  const uint32_t from = p0 < 0 ? 0u : (uint32_t)p0, to = p0 + 16 < (int64_t)total ? (uint32_t)(p0 + 16) : total;
  uint32_t i = find_le(seg, 0u, n - 1u, from);  // the segment that holds `from`: seg[0] = 0 <= from
  ScafSeg m = scaf_seg_load<FILL>(members, seg, fill, offs, i);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int64_t p = p0 + j;
    uint32_t c = 0;
    if (p >= (int64_t)from && p < (int64_t)to) {
      while ((uint32_t)p >= m.s1) m = scaf_seg_load<FILL>(members, seg, fill, offs, ++i);  // ends: seg[n] = total > p
      const uint32_t q = (uint32_t)p - m.s0;
      if (q < m.nrun)
        c = FILL && m.fill != SCAF_NONE ? (uint32_t)buf[m.fill + q] : (uint32_t)'N';
      else {
        const uint32_t b = q - m.nrun + m.skip;
        c = b < m.len ? scaf_text(src + m.base, m.len, m.rev, b) : (uint32_t)'_';
      }
    }
    w[j >> 2] |= c << (8 * (j & 3));
  }
  if (to - from == 16u)
    *(uint4 *)(out + p0) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      if (p >= (int64_t)from && p < (int64_t)to) out[p] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

__global__ void __launch_bounds__(SCAF_TPB) kc_scaf_write_kernel(const uint4 *members, const uint32_t *seg, uint32_t n, const uint8_t *src,
                                                                 const uint32_t *offs, uint32_t mis, uint32_t total, uint8_t *out) {
  scaf_write_body<false>(members, seg, nullptr, n, src, offs, nullptr, mis, total, out);
}

}  // namespace kc
