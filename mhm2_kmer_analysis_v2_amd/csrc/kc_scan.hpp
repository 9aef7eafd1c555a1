// kc_scan.hpp -- the front end's one scan: a single workgroup turns per-tile sums into exclusive offsets, in place.
// The FASTQ parser scans its tile line counts and its per-workgroup sequence sums with it, the trim its per-tile bytes
// (NA = 1), the pair merge its per-tile bytes and reads in one pass (NA = 2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kc {

constexpr int SCAN_TPB = 1024;
constexpr int SCAN_ITEMS = 8;  // consecutive items a thread takes per round

// the arrays of one launch, by value in the kernel arguments: the loops over a < NA have constant bounds and unroll, so
// every index into v is a compile-time constant and the pointers stay in scalar registers (no scratch: the resource
// test checks it)
template <int NA>
struct ScanArrays {
  uint64_t *v[NA];
};

// exclusive scan of v[a][0, n) in place for every a < NA; totals[a] = the sum of array a
template <int NA>
__global__ void __launch_bounds__(SCAN_TPB) kc_scan_kernel(ScanArrays<NA> arr, uint64_t n, uint64_t *totals) {
  __shared__ uint64_t ws[SCAN_TPB / 64][NA];
  __shared__ uint64_t carry[NA];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0)
    for (int a = 0; a < NA; a++) carry[a] = 0;
  __syncthreads();
  for (uint64_t base = 0; base < n; base += (uint64_t)SCAN_TPB * SCAN_ITEMS) {
    const uint64_t first = base + (uint64_t)tid * SCAN_ITEMS;
    uint64_t x[NA][SCAN_ITEMS], s[NA], inc[NA], p[NA];
    for (int a = 0; a < NA; a++) s[a] = 0;
    for (int k = 0; k < SCAN_ITEMS; k++) {
      const bool in = first + k < n;
      if (in)  // one predicate for the NA loads of an item, and below for its stores
        for (int a = 0; a < NA; a++) x[a][k] = arr.v[a][first + k];
      else
        for (int a = 0; a < NA; a++) x[a][k] = 0;
      for (int a = 0; a < NA; a++) s[a] += x[a][k];
    }
    for (int a = 0; a < NA; a++) inc[a] = s[a];  // inclusive within the wave
    for (int o = 1; o < 64; o <<= 1) {
      uint64_t t[NA];
      for (int a = 0; a < NA; a++) t[a] = __shfl_up(inc[a], o);
      const bool up = lane >= o;
      for (int a = 0; a < NA; a++) inc[a] += up ? t[a] : 0;
    }
    if (lane == 63)
      for (int a = 0; a < NA; a++) ws[wv][a] = inc[a];
    __syncthreads();
    for (int a = 0; a < NA; a++) p[a] = carry[a];
    for (int w = 0; w < wv; w++)
      for (int a = 0; a < NA; a++) p[a] += ws[w][a];
    for (int a = 0; a < NA; a++) p[a] += inc[a] - s[a];
    for (int k = 0; k < SCAN_ITEMS; k++) {
      if (first + k < n)
        for (int a = 0; a < NA; a++) arr.v[a][first + k] = p[a];
      for (int a = 0; a < NA; a++) p[a] += x[a][k];
    }
    __syncthreads();
    if (tid == SCAN_TPB - 1)
      for (int a = 0; a < NA; a++) carry[a] = p[a];
    __syncthreads();
  }
  if (tid == 0)
    for (int a = 0; a < NA; a++) totals[a] = carry[a];
}

}  // namespace kc
