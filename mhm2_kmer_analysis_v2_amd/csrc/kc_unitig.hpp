// kc_unitig.hpp -- unitigs from the results: the unique-extension paths of the de Bruijn graph the results describe,
// built on the device (kc_build_unitigs).  DESIGN.md section 14 holds the definition; it is this project's own (the
// reference's traversal is commented out in the proxy), pinned by the host model tests/unitig_model.py.
//
// The results are in key order (kc_sort_results), so "the smaller canonical k-mer" is the smaller result number.  An
// oriented node is v = 2 * result + strand (0: the k-mer as stored, 1: its reverse complement); twin(v) = v ^ 1;
// UNITIG_NONE = no node.  Every node has at most one successor and one predecessor, v -> w iff twin(w) -> twin(v), and
// no component is its own twin, so the components are simple paths and cycles.
//
//  kc_unitig_links_kernel<NL>  a thread per result: the successors of (i,+) and (i,-) -- shift the extension in,
//                              canonicalise, probe the lookup index (kc_index_find), check the link's four conditions.
//                              Writes next[] and the first buffer of the cycle search {next, result number}.
//  kc_unitig_min_jump_kernel   one round of pointer jumping along next[], carrying the smallest result number seen:
//                              {p, m}[v] <- {p[p[v]], min(m[v], m[p[v]])}, from one buffer into the other.  After
//                              ceil(log2 2n) + 1 rounds every node of a path has run off its end; what still has a
//                              pointer lies on a cycle and knows the cycle's smallest result number.
//  kc_unitig_cut_kernel        a thread per result: cuts a cycle in front of (x*,+) and its twin behind (x*,-), in next[],
//                              and writes the first buffer of the ranking {predecessor or itself, 1 or 0}
//                              (pred(v) = twin(next(twin(v))): both are the thread's own two entries).
//  kc_unitig_rank_jump_kernel  one round along the predecessors: {p, d}[v] <- {p[p[v]], d[v] + d[p[v]]}; a head points at
//                              itself with distance 0, so it is a fixed point and needs no test.  Afterwards p is the
//                              head and d the distance from it.
//  kc_unitig_select_kernel     a thread per node; the tail of a path (no successor) knows m = d + 1, its head, and the head
//                              of the twin path (its own twin): the path whose head is the smaller result is the one
//                              emitted, and the tail writes k + m bytes, one unitig and the head's strand at the head's
//                              result number.  kc_scan_kernel<2> over result order makes them text offsets and unitig
//                              numbers: unitigs come out in the order of their heads' keys.
//  kc_unitig_write_kernel      a thread per node of an emitted path: the head writes its k bases and its offset, the
//                              node at distance d its last base at offset + k - 1 + d, the tail the separator; every
//                              node adds its count to the unitig's sum (a 64-bit atomic add: integer, so the order of
//                              arrival does not show).
//  kc_unitig_depth_kernel      a thread per node again: the depth of the unitig on the node's bytes, 0 on the separator.
//
// No kernel here has a loop whose trip count depends on a chain's length or on another thread: a round is a launch, the
// host fixes the number of rounds from n, and a round reads one buffer and writes the other.  The only data-dependent
// loop is the index probe, which ends at an empty slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_kernels.hpp"
#include "kc_kit.hpp"

namespace kc {

constexpr uint32_t UNITIG_NONE = 0xFFFFFFFFu;
constexpr int UNITIG_TPB = 256;
// device statistics of a call (uint64_t each)
enum { UST_CIRCULAR = 0, UST_SINGLETONS, UST_LONGEST, UST_TOTALS, UST_COUNT = UST_TOTALS + 2 };  // totals: bytes, unitigs

// the thread's item, and whether it has one: the last workgroup of 2^32 - 2 nodes reaches past 32 bits
__device__ __forceinline__ bool unitig_thread(uint32_t items, uint32_t &t) {
  const uint64_t g = (uint64_t)blockIdx.x * UNITIG_TPB + threadIdx.x;
  t = (uint32_t)g;
  return g < items;
}

// The node that the node with sequence sq (x, or its reverse complement) and right extension `code` links to.
template <int NL>
__device__ __forceinline__ uint32_t unitig_successor(const uint64_t (&sq)[NL], uint32_t code, const uint64_t (&x)[NL], int k,
                                                     const uint32_t *index, uint64_t mask, const uint64_t *keys, const uint8_t *left,
                                                     const uint8_t *right) {
  uint64_t w[NL], r[NL], y[NL];
  const int lw = (k - 1) >> 5, sh = 62 - 2 * ((k - 1) & 31);
#pragma unroll
  for (int j = 0; j < NL; j++) {  // (bits behind base k - 1 are zero in sq, so the slot of the new base comes out empty)
    w[j] = (sq[j] << 2) | (j + 1 < NL ? sq[j + 1] >> 62 : 0ULL);
    if (j == lw) w[j] |= (uint64_t)code << sh;
  }
  kc_revcomp<NL>(w, k, r);
  const bool fwd = !kc_less<NL>(r, w);  // w is the canonical one: the link arrives at (y,+)
  bool pal = true, self = true;
#pragma unroll
  for (int j = 0; j < NL; j++) {
    y[j] = fwd ? w[j] : r[j];
    pal &= w[j] == r[j];
    self &= y[j] == x[j];
  }
  if (pal || self) return UNITIG_NONE;
  const uint32_t e = kc_index_find<NL>(y, index, mask, keys);
  if (!e) return UNITIG_NONE;
  // both sides agree: extL(y,+) = left(y), extL(y,-) = comp(right(y)) must be the first base of sq
  const uint32_t first = (uint32_t)(sq[0] >> 62);
  const uint32_t have = fwd ? left[e - 1] : right[e - 1];
  if (have != code_letter(fwd ? first : 3u - first)) return UNITIG_NONE;
  return 2u * (e - 1u) + (fwd ? 0u : 1u);
}

// next2[i] = {next(i,+), next(i,-)}; cyc4[i] = {next(i,+), i, next(i,-), i}
template <int NL>
__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_links_kernel(const uint64_t *keys, const uint8_t *left, const uint8_t *right, uint32_t n,
                                                                     int k, const uint32_t *index, uint64_t mask, uint2 *next2, uint4 *cyc4) {
  uint32_t i;
  if (!unitig_thread(n, i)) return;
  uint64_t f[NL], r[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) f[j] = keys[(uint64_t)i * NL + j];
  kc_revcomp<NL>(f, k, r);
  bool pal = true;
#pragma unroll
  for (int j = 0; j < NL; j++) pal &= f[j] == r[j];
  const uint32_t lc = left[i], rc = right[i];
  uint32_t n0 = UNITIG_NONE, n1 = UNITIG_NONE;
  if (!pal) {  // a k-mer that is its own reverse complement (even k) is a unitig of its own
    if (kc_is_acgt(rc)) n0 = unitig_successor<NL>(f, kc_base_code(rc), f, k, index, mask, keys, left, right);
    if (kc_is_acgt(lc)) n1 = unitig_successor<NL>(r, 3u - kc_base_code(lc), f, k, index, mask, keys, left, right);
  }
  next2[i] = make_uint2(n0, n1);
  cyc4[i] = make_uint4(n0, i, n1, i);
}

__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_min_jump_kernel(const uint2 *in, uint2 *out, uint32_t nn) {
  uint32_t v;
  if (!unitig_thread(nn, v)) return;
  uint2 e = in[v];
  if (e.x != UNITIG_NONE) {
    const uint2 a = in[e.x];
    e.x = a.x;
    e.y = min(e.y, a.y);
  }
  out[v] = e;
}

// cyc4: the cycle search's last buffer.  A node that still has a pointer there lies on a cycle whose smallest result is
// its .y: the link into (x*,+) goes, and so does the link out of (x*,-), which is the same cut on the twin cycle.
__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_cut_kernel(const uint4 *cyc4, uint2 *next2, uint4 *rank4, uint32_t n, uint64_t *st) {
  uint32_t i, circ = 0;
  if (unitig_thread(n, i)) {
    uint2 nx = next2[i];
    const uint4 c = cyc4[i];
    if (c.x != UNITIG_NONE && nx.x == 2u * c.y) nx.x = UNITIG_NONE;
    if (c.z != UNITIG_NONE) {
      if (nx.y == 2u * c.w || c.w == i) nx.y = UNITIG_NONE;
      circ = c.w == i;  // once per cycle and twin
    }
    next2[i] = nx;
    // pred(i,+) = twin(next(i,-)), pred(i,-) = twin(next(i,+)); a head points at itself
    rank4[i] = make_uint4(nx.y != UNITIG_NONE ? nx.y ^ 1u : 2u * i, nx.y != UNITIG_NONE, nx.x != UNITIG_NONE ? nx.x ^ 1u : 2u * i + 1u,
                          nx.x != UNITIG_NONE);
  }
  circ = wave_sum(circ);
  if ((threadIdx.x & 63) == 0 && circ) atomicAdd((unsigned long long *)&st[UST_CIRCULAR], (unsigned long long)circ);
}

__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_rank_jump_kernel(const uint2 *in, uint2 *out, uint32_t nn) {
  uint32_t v;
  if (!unitig_thread(nn, v)) return;
  const uint2 e = in[v], a = in[e.x];
  out[v] = make_uint2(a.x, e.y + a.y);
}

// rank: {head, distance} of every node.  size, num, sel: zeroed, one entry a result.
__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_select_kernel(const uint2 *rank, const uint32_t *next, uint32_t nn, int k, uint64_t *size,
                                                                      uint64_t *num, uint8_t *sel, uint64_t *st) {
  uint32_t v, single = 0;
  unsigned long long len = 0;
  if (unitig_thread(nn, v) && next[v] == UNITIG_NONE) {  // a tail
    const uint2 e = rank[v];
    const uint32_t h = e.x;
    // the twin path's head is twin(v): of the two, the path whose head is the smaller result; a lone k-mer as (x,+)
    if ((h >> 1) < (v >> 1) || (h == v && !(v & 1u))) {
      size[h >> 1] = (uint64_t)k + e.y + 1u;  // k + m - 1 bases and the separator
      num[h >> 1] = 1;
      sel[h >> 1] = (uint8_t)(1u + (h & 1u));
      single = e.y == 0u;
      len = (unsigned long long)k + e.y;
    }
  }
  single = wave_sum(single);
  len = wave_max(len);
  if ((threadIdx.x & 63) == 0) {
    if (single) atomicAdd((unsigned long long *)&st[UST_SINGLETONS], (unsigned long long)single);
    if (len) atomicMax((unsigned long long *)&st[UST_LONGEST], len);
  }
}

// off, unum: size and num after the scan.  total, nu: bytes and unitigs of the whole (offsets[nu] = total).
// sums (may be null): zeroed, one entry a unitig.
__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_write_kernel(const uint2 *rank, const uint32_t *next, const uint64_t *keys, int nl,
                                                                     const uint16_t *counts, const uint8_t *sel, const uint64_t *off,
                                                                     const uint64_t *unum, uint32_t nn, int k, uint64_t total, uint64_t nu,
                                                                     uint8_t *seqs, uint64_t *offsets, uint64_t *sums) {
  uint32_t v;
  if (!unitig_thread(nn, v)) return;
  if (v == 0) offsets[nu] = total;
  const uint2 e = rank[v];
  const uint32_t hi = e.x >> 1;
  if (sel[hi] != 1u + (e.x & 1u)) return;  // the twin of an emitted path
  const uint64_t at = off[hi], u = unum[hi];
  const uint64_t *kw = keys + (uint64_t)(v >> 1) * nl;
  const bool rev = v & 1u;
  if (e.y == 0u) {  // the head: seq(v), base j of the reverse complement being the complement of base k - 1 - j
    offsets[u] = at;
    uint64_t word = 0;
    int have = -1;
    for (int j = 0; j < k; j++) {
      const int src = rev ? k - 1 - j : j;
      if ((src >> 5) != have) {
        have = src >> 5;
        word = kw[have];
      }
      const uint32_t code = (uint32_t)(word >> (62 - 2 * (src & 31))) & 3u;
      if (at + j < total) seqs[at + j] = (uint8_t)code_letter(rev ? 3u - code : code);
    }
  } else {  // the last base of seq(v)
    const uint32_t code = rev ? 3u - (uint32_t)(kw[0] >> 62) : (uint32_t)(kw[(k - 1) >> 5] >> (62 - 2 * ((k - 1) & 31))) & 3u;
    const uint64_t p = at + (uint64_t)k - 1u + e.y;
    if (p < total) seqs[p] = (uint8_t)code_letter(code);
  }
  if (next[v] == UNITIG_NONE) {
    const uint64_t p = at + (uint64_t)k + e.y;
    if (p < total) seqs[p] = '_';
  }
  if (sums) atomicAdd((unsigned long long *)&sums[u], (unsigned long long)counts[v >> 1]);
}

// depth = min(65535, (2 * sum + m) / (2 * m)): the mean count, rounded half up
__global__ void __launch_bounds__(UNITIG_TPB) kc_unitig_depth_kernel(const uint2 *rank, const uint32_t *next, const uint8_t *sel,
                                                                     const uint64_t *off, const uint64_t *unum, const uint64_t *offsets,
                                                                     const uint64_t *sums, uint32_t nn, int k, uint64_t total, uint16_t *depths) {
  uint32_t v;
  if (!unitig_thread(nn, v)) return;
  const uint2 e = rank[v];
  const uint32_t hi = e.x >> 1;
  if (sel[hi] != 1u + (e.x & 1u)) return;
  const uint64_t at = off[hi], u = unum[hi];
  const uint64_t m = offsets[u + 1] - at - (uint64_t)k;
  const uint64_t mean = (2u * sums[u] + m) / (2u * m);
  const uint16_t dep = (uint16_t)(mean < 65535u ? mean : 65535u);
  if (e.y == 0u) {
    for (int j = 0; j < k; j++)
      if (at + j < total) depths[at + j] = dep;
  } else {
    const uint64_t p = at + (uint64_t)k - 1u + e.y;
    if (p < total) depths[p] = dep;
  }
  if (next[v] == UNITIG_NONE) {
    const uint64_t p = at + (uint64_t)k + e.y;
    if (p < total) depths[p] = 0;
  }
}

}  // namespace kc
