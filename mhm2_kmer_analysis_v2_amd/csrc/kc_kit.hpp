// kc_kit.hpp -- the small helpers the contig-pass and text kernel headers share (kc_unitig.hpp, kc_sort.hpp, kc_align.hpp
// and everything behind them): one definition each of the search, the decimal text, the base codes, the wave reductions,
// the workgroup counters and the segmented scan.  A new kernel header takes these from here and adds no copy of its own
// (DESIGN.md section 28).  The counting path (kc_kernels.hpp, kc_bucketed.hpp and their kin) keeps its own loops.
//
// The first part is plain arithmetic, KC_HD like kc_common.hpp: a host compiler builds it, and tests/cpp/test_kit.cpp
// holds it to the definitions it replaced.  The second part needs the wave and is device code only.
#pragma once
#include "kc_common.hpp"

namespace kc {

// ---- pure helpers ----------------------------------------------------------------------------------------------------
// The greatest j in [lo, hi] with at(j) <= x, for an at() that never decreases and at(lo) <= x (given, never read).  The
// same call answers "which item holds x" for n items with at(0) <= x: find_le(0, n - 1, ...), and one more is the first
// item that starts behind x.
template <class I, class X, class At>
KC_HD I find_le(I lo, I hi, X x, At at) {
  while (lo < hi) {
    const I mid = lo + ((hi - lo + 1) >> 1);
    if (at(mid) <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}
template <class T, class I, class X>
KC_HD I find_le(const T *a, I lo, I hi, X x) {
  return find_le(lo, hi, x, [a](I mid) { return a[mid]; });
}

// the decimal digits of v, of which the caller knows there are at most MAXD (a greater v counts MAXD)
// as a chain of MAXD - 1 compares: v < 10 ? 1 : v < 100 ? 2 : ... : MAXD
template <int MAXD, int D = 1, class T>
KC_HD uint32_t dec_digits(T v, T p = 10) {
  if constexpr (D >= MAXD)
    return (uint32_t)MAXD;
  else
    return v < p ? (uint32_t)D : dec_digits<MAXD, D + 1>(v, (T)(p * 10));
}

// the decimal digits of v, four bits each, the last digit lowest (sixteen digits fit)
template <class T>
KC_HD uint64_t dec_bcd(T v) {
  uint64_t bcd = 0;
  int s = 0;
  do {
    bcd |= (uint64_t)(v % 10u) << s;
    v /= 10u;
    s += 4;
  } while (v);
  return bcd;
}

// A C G T of either case as 0 .. 3, every other byte 4
KC_HD uint32_t base_code4(uint32_t c) {
  c &= 0xDFu;  // a letter's upper case; no other byte becomes one of the four
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// the complement of an upper-case A C G T; every other byte as it is
KC_HD uint32_t base_comp(uint32_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// code 0 .. 3 as its letter
KC_HD uint32_t code_letter(uint32_t code) { return (0x54474341u >> (8 * code)) & 0xFFu; }  // "ACGT"

#if defined(__HIPCC__)
// ---- the wave and the workgroup --------------------------------------------------------------------------------------
// Every lane of the wave calls these and every lane holds the result.  T: a 32- or 64-bit integer; a 64-bit value costs
// two shuffles a step, so a site passes the width it needs.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
  for (int o = 32; o; o >>= 1) {
    const T t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
  for (int o = 32; o; o >>= 1) {
    const T t = __shfl_xor(v, o);
    v = t < v ? t : v;
  }
  return v;
}

// the same butterfly over a structure S with S across(int o) const (the lane o away's) and S join(const S &other) const
template <class S>
__device__ __forceinline__ S wave_join(S s) {
  for (int o = 32; o; o >>= 1) s = s.join(s.across(o));
  return s;
}

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// st[k] += the wave's sum of v: one atomic a wave, none for a sum of zero
__device__ __forceinline__ void wave_add(uint64_t *st, int k, unsigned long long v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long *)&st[k], v);
}

// NK counters of a workgroup: wave sums into LDS, then one global atomic a workgroup and counter.  Every wave of the call
// adding to one address is what a counter costs (0.15 ms for 15 000 waves); the statistics kernels run 1024 threads a
// workgroup for the same reason.  Every thread of the workgroup calls it; a workgroup's sums fit 32 bits.
template <int NK>
__device__ __forceinline__ void wg_stats(uint64_t *st, const int (&k)[NK], const uint32_t (&mine)[NK]) {
  __shared__ uint32_t sums[NK];
  if ((int)threadIdx.x < NK) sums[threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NK; j++) {
    uint32_t v = mine[j];  // wave_sum's loop written out: through the call the NK sums interleave and take half as many registers again
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sums[j], v);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NK; j++)
    if ((int)threadIdx.x == j && sums[j]) atomicAdd((unsigned long long *)&st[k[j]], (unsigned long long)sums[j]);
}

// The wave's segmented inclusive scan: f marks a lane that starts a segment; s becomes the join of its segment's lanes up
// to and with its own.  S has S up(int o) const (the value o lanes below) and S join(const S &later) const.
template <class S>
__device__ __forceinline__ void wave_seg_scan(S &s, bool f, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const S t = s.up(o);
    const bool tf = __shfl_up((int)f, o) != 0;
    if (lane >= o) {
      if (!f) s = t.join(s);
      f = f || tf;
    }
  }
}
#endif  // __HIPCC__

}  // namespace kc
