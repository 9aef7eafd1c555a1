// kc_sort.hpp -- the back end of the results: order them by key, and write the reference's dump text, on the device.
//
// Replaces what a consumer of KmerDHT::dump_kmers (src/kcount/kmer_dht.cpp:273-297) does on the host today: the reference
// walks its hash map (any order) and prints "KMER count L R" lines; everything that compares two dumps sorts them first.
//
// The sort is a stable LSD radix sort of a 32-bit PERMUTATION, eight bits a pass, over the 2k significant bits of a key
// only: word w holds min(64, 2k - 64w) of them at its top (S3), so a pass starts at bit 64 - that and the last digit of a
// word may be partial (k = 21: five digits of eight bits and one of two); a word without significant bits (the last at
// k = 32, 64, 96) gets no pass.  Words are taken from the last to the first.  The current word travels beside the
// index (key word and index: twelve bytes an item), so the passes of a word read nothing at random; the first pass of a
// word gathers it through the index once, inside that pass's histogram kernel.
//
// A pass, over tiles of SORT_TILE items:
//  kc_sort_hist_kernel     a workgroup per tile: digit histogram in LDS, written digit-major (cnt[digit * ntiles + tile]),
//                          so that ONE exclusive scan of the whole array (kc_scan_kernel<1>, kc_scan.hpp) turns every
//                          counter into the global position of that tile's first item with that digit.  <LOAD>: the
//                          first pass of a word also gathers the word through the index and stores it beside it.
//  kc_sort_scatter_kernel  a workgroup per tile, a wave per quarter of it in order.  Sixteen rounds of 64 items: eight
//                          ballots find a lane's peers (same digit), the first peer adds their number to the
//                          (wave, digit) counter in LDS, a lane's rank is that counter before plus its place among the
//                          peers -- kept in LDS (u16), the keys in registers.  256 threads then turn the 4 x 256 counters
//                          into starts within the tile (digit-major, waves in order inside a digit: stable), the items
//                          go to their place in an LDS copy of the tile, and the copy is written out in digit order:
//                          consecutive threads store consecutive items of a digit's run.
// After the last pass kc_sort_gather_kernel writes keys (both widths where the library keeps two), counts, left and
// right through the permutation into fresh arrays.
//
// The text: a line is k bases, ' ', the count in decimal (1..5 digits), ' ', L, ' ', R = k + 5 + digits bytes, and '\n'.
//  kc_dump_sizes_kernel    a workgroup per tile of DUMP_TILE lines: the tile's bytes from its counts' digit numbers;
//                          kc_scan_kernel<1> makes them offsets and the total (a size query ends here).
//  kc_dump_write_kernel    a workgroup per tile: a thread composes its line in LDS, at the place the line has in the
//                          tile, the whole shifted by the destination's misalignment, so that LDS and HBM addresses agree
//                          modulo 16; the tile then leaves as 16-byte stores, lane after lane, with byte stores only for
//                          the ragged head and tail.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_kit.hpp"

namespace kc {

constexpr int SORT_TILE = 4096;  // items per workgroup and pass
constexpr int SORT_TPB = 256;
constexpr int SORT_WAVES = SORT_TPB / 64;
constexpr int SORT_ROUNDS = SORT_TILE / SORT_TPB;  // rounds of 64 items per wave
constexpr int SORT_BITS = 8;
constexpr int SORT_DIGITS = 1 << SORT_BITS;
static_assert(SORT_DIGITS == SORT_TPB, "one thread per digit turns the counters into starts");

constexpr int DUMP_TILE = 256;  // lines per workgroup
constexpr int DUMP_MAX_K = 125;
constexpr int DUMP_MAX_LINE = DUMP_MAX_K + 5 + 5 + 1;  // five digits, the newline

// digit of a key word in a pass: `bits` bits from `shift` on
__device__ __forceinline__ uint32_t sort_digit(uint64_t word, int shift, uint32_t mask) { return (uint32_t)(word >> shift) & mask; }

// Per-tile digit counts, digit-major.  idx == nullptr: the identity (the first pass of all).  LOAD: the word comes from
// keys[item * nl + w] through the index and is stored to kbuf for the scatter and the later passes of the word; else it
// is read from kbuf.
template <bool LOAD>
__global__ void __launch_bounds__(SORT_TPB) kc_sort_hist_kernel(const uint64_t *keys, int nl, int w, const uint32_t *idx, uint64_t *kbuf,
                                                                uint64_t n, uint64_t ntiles, int shift, uint32_t mask, uint64_t *cnt) {
  __shared__ uint32_t hist[SORT_DIGITS];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint64_t i = base + (uint64_t)r * SORT_TPB + tid;
    if (i < n) {
      uint64_t word;
      if (LOAD) {
        const uint64_t src = idx ? (uint64_t)idx[i] : i;
        word = keys[src * nl + w];
        kbuf[i] = word;
      } else {
        word = kbuf[i];
      }
      atomicAdd(&hist[sort_digit(word, shift, mask)], 1u);
    }
  }
  __syncthreads();
  cnt[(uint64_t)tid * ntiles + blockIdx.x] = hist[tid];
}

// One pass's move: (kin, iin) -> (kout, iout), stable.  cnt: the scanned counters.  iin == nullptr: the identity.
__global__ void __launch_bounds__(SORT_TPB) kc_sort_scatter_kernel(const uint64_t *kin, const uint32_t *iin, uint64_t *kout, uint32_t *iout,
                                                                   uint64_t n, uint64_t ntiles, int shift, uint32_t mask, const uint64_t *cnt) {
  __shared__ uint64_t skey[SORT_TILE];
  __shared__ uint32_t sidx[SORT_TILE];
  __shared__ uint16_t rank[SORT_TILE];
  __shared__ uint32_t wcnt[SORT_WAVES][SORT_DIGITS];
  __shared__ uint64_t gbase[SORT_DIGITS];  // global position of the tile's first item of a digit, less its place in the tile
  __shared__ uint32_t wsum[SORT_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
  const uint32_t here = (uint32_t)(n - base < (uint64_t)SORT_TILE ? n - base : (uint64_t)SORT_TILE);
  for (int w = 0; w < SORT_WAVES; w++) wcnt[w][tid] = 0;
  __syncthreads();
  // ranks: a wave takes items [wv * 1024, +1024) in rounds of 64
  uint64_t key[SORT_ROUNDS];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t it = (uint32_t)(wv * (SORT_TILE / SORT_WAVES) + r * 64 + lane);
    const bool valid = it < here;
    key[r] = valid ? kin[base + it] : 0;
    const uint32_t d = sort_digit(key[r], shift, mask);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < SORT_BITS; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    uint32_t before = 0;
    const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
    if (valid && lane == leader) before = atomicAdd(&wcnt[wv][d], (uint32_t)__popcll(peers));
    before = __shfl(before, leader);
    if (valid) rank[it] = (uint16_t)(before + (uint32_t)__popcll(peers & below));
  }
  __syncthreads();
  // thread = digit: the waves' counts become starts within the tile, digit after digit, wave after wave
  {
    uint32_t c[SORT_WAVES], total = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; w++) {
      c[w] = wcnt[w][tid];
      total += c[w];
    }
    uint32_t inc = total;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t start = inc - total;
    for (int w = 0; w < wv; w++) start += wsum[w];
    gbase[tid] = cnt[(uint64_t)tid * ntiles + blockIdx.x] - start;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; w++) {
      wcnt[w][tid] = start;
      start += c[w];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t it = (uint32_t)(wv * (SORT_TILE / SORT_WAVES) + r * 64 + lane);
    if (it < here) {
      const uint32_t pos = wcnt[wv][sort_digit(key[r], shift, mask)] + rank[it];
      skey[pos] = key[r];
      sidx[pos] = iin ? iin[base + it] : (uint32_t)(base + it);
    }
  }
  __syncthreads();
  for (uint32_t j = tid; j < here; j += SORT_TPB) {
    const uint64_t k = skey[j];
    const uint64_t dst = gbase[sort_digit(k, shift, mask)] + j;
    if (dst < n) {  // always, while the counters are those of these keys
      kout[dst] = k;
      iout[dst] = sidx[j];
    }
  }
}

// the result arrays through the permutation; keys_ext (may be null): the same keys at the reference's width
__global__ void __launch_bounds__(256) kc_sort_gather_kernel(const uint32_t *perm, uint64_t n, int nl, const uint64_t *keys, uint64_t *keys_out,
                                                            int nl_ext, const uint64_t *ext, uint64_t *ext_out, const uint16_t *counts,
                                                            uint16_t *counts_out, const uint8_t *left, uint8_t *left_out, const uint8_t *right,
                                                            uint8_t *right_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = perm[i];
  for (int j = 0; j < nl; j++) keys_out[i * nl + j] = keys[s * nl + j];
  if (ext)
    for (int j = 0; j < nl_ext; j++) ext_out[i * nl_ext + j] = ext[s * nl_ext + j];
  counts_out[i] = counts[s];
  left_out[i] = left[s];
  right_out[i] = right[s];
}

// ---- the dump text ---------------------------------------------------------------------------------------------------
// bytes of the lines of entries [first + tile * DUMP_TILE, ...) of [first, first + count)
__global__ void __launch_bounds__(DUMP_TILE) kc_dump_sizes_kernel(const uint16_t *counts, uint64_t first, uint64_t count, int k,
                                                                  uint64_t *tile_bytes) {
  __shared__ uint32_t ws[DUMP_TILE / 64];
  const int tid = threadIdx.x;
  const uint64_t e = (uint64_t)blockIdx.x * DUMP_TILE + tid;
  const uint32_t len = wave_sum(e < count ? (uint32_t)k + 6u + dec_digits<5>((uint32_t)counts[first + e]) : 0u);
  if ((tid & 63) == 0) ws[tid >> 6] = len;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
    for (int w = 0; w < DUMP_TILE / 64; w++) s += ws[w];
    tile_bytes[blockIdx.x] = s;
  }
}

// tile_off: the scanned tile_bytes.  keys: nl words an entry, the reference's width.
__global__ void __launch_bounds__(DUMP_TILE) kc_dump_write_kernel(const uint64_t *keys, int nl, const uint16_t *counts, const uint8_t *left,
                                                                  const uint8_t *right, uint64_t first, uint64_t count, int k,
                                                                  const uint64_t *tile_off, uint8_t *text) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[DUMP_TILE * DUMP_MAX_LINE + 16];
  __shared__ uint32_t ws[DUMP_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t e = (uint64_t)blockIdx.x * DUMP_TILE + tid;
  const bool in = e < count;
  const uint32_t c = in ? counts[first + e] : 0u;
  const uint32_t nd = dec_digits<5>(c);
  const uint32_t len = in ? (uint32_t)k + 6u + nd : 0u;
  uint32_t inc = len;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  uint32_t off = inc - len, total = 0;
  for (int w = 0; w < DUMP_TILE / 64; w++) {
    if (w < wv) off += ws[w];
    total += ws[w];
  }
  uint8_t *dst = text + tile_off[blockIdx.x];
  const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);  // the tile sits in buf as it will in memory, modulo 16
  if (in) {
    uint8_t *p = buf + mis + off;
    const uint64_t *kw = keys + (first + e) * nl;
    uint64_t word = 0;
    for (int i = 0; i < k; i++) {
      if ((i & 31) == 0) word = kw[i >> 5];
      const uint32_t code = (uint32_t)(word >> 62);
      word <<= 2;
      p[i] = (uint8_t)code_letter(code);
    }
    p += k;
    *p++ = ' ';
    uint32_t v = c;
    for (uint32_t j = nd; j-- > 0;) {
      p[j] = (uint8_t)('0' + v % 10u);
      v /= 10u;
    }
    p += nd;
    p[0] = ' ';
    p[1] = left[first + e];
    p[2] = ' ';
    p[3] = right[first + e];
    p[4] = '\n';
  }
  __syncthreads();
  uint32_t head = (16u - mis) & 15u;
  if (head > total) head = total;
  if ((uint32_t)tid < head) dst[tid] = buf[mis + tid];
  const uint32_t nvec = (total - head) >> 4;
  const uint4 *s16 = (const uint4 *)(buf + mis + head);  // mis + head is 0 or 16
  uint4 *d16 = (uint4 *)(dst + head);
  for (uint32_t v = tid; v < nvec; v += DUMP_TILE) d16[v] = s16[v];
  const uint32_t done = head + (nvec << 4);
  if (done + (uint32_t)tid < total) dst[done + tid] = buf[mis + done + tid];
}

}  // namespace kc
