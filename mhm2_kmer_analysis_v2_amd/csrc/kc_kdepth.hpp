// kc_kdepth.hpp -- two readers of the finished results: the k-mer depth of sequences (kc_seq_kmer_depths) and the histogram of
// the results' counts (kc_count_spectrum).  DESIGN.md section 31 holds the rules; they are this project's own (the reference
// asks the table k-mer by k-mer, src/kcount/kmer_dht.cpp:198-245), pinned by the host model tests/kdepth_model.py.
//
//  kc_ktrack_offsets_kernel        a thread per sequence: offsets that do not decrease, start at 0 and end at nbytes, no
//                                  sequence of 2^32 bytes; the longest sequence.  (kc_align_lengths_kernel refuses anything
//                                  over 1024 bytes, which contigs are, so it cannot serve here.)
//  kc_ktrack_windows_kernel<NL, FILL>  a lane owns KT_RUN consecutive positions.  It finds the sequence of its first one once
//                                  (find_le over the offsets), then reads KT_RUN + k - 1 bytes and rolls the forward and the
//                                  reverse-complement words one base a step; a counter of consecutive bases since the last
//                                  non-base or sequence start says whether the k bytes that end here are a window.  KT_FLIGHT
//                                  windows are canonicalised and hashed, then their index slots, key words and counts are
//                                  loaded side by side: the three loads of a probe depend on each other, those of different
//                                  windows do not.  A lane sums what its windows give while it stays in one sequence; at the
//                                  end a wave whose lanes all stand in one sequence reduces and adds once, other lanes add
//                                  for themselves.  The call's totals go through wg_stats.
//  kc_ktrack_records_kernel        a thread per sequence: the sums become kc_kdepth_rec and the mean.
//  kc_ktrack_fill_kernel           (KC_KDEPTH_FILL_MEAN) a lane owns 8 values of the track: its sequence's mean on a base,
//                                  0 on any other byte.
//  kc_spect_hist_kernel            counts below SPECT_LOW go to a workgroup's LDS histogram, SPECT_REP copies of it picked
//                                  by the lane so that equal counts do not all meet at one address; the rare others go to
//                                  64-bit global atomics.  Only bins that are not zero are flushed.
//  kc_spect_stats_kernel           one workgroup over the 65536 bins: k-mers, sum, greatest count, mode, saturated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_kernels.hpp"
#include "kc_kit.hpp"

namespace kc {

constexpr int KT_TPB = 256;
#ifndef KC_KTRACK_RUN
#define KC_KTRACK_RUN 16
#endif
#ifndef KC_KTRACK_FLIGHT
#define KC_KTRACK_FLIGHT 4
#endif
constexpr int KT_RUN = KC_KTRACK_RUN;        // positions a lane owns
constexpr int KT_FLIGHT = KC_KTRACK_FLIGHT;  // windows whose probes are in flight together
constexpr int KT_FILL_ITEMS = 8;             // values of the track a lane of the fill kernel writes: 16 bytes
static_assert(KT_RUN % KT_FLIGHT == 0 && KT_RUN * 65535ull * KT_TPB < (1ull << 32), "a workgroup's sums fit 32 bits (wg_stats)");

enum { KTS_BAD = 0, KTS_LONG, KTS_ENDS, KTS_LONGEST, KTS_WINDOWS, KTS_PRESENT, KTS_SOLID, KTS_SUM, KTS_COUNT };

// what the windows of one sequence add up to; all zero before the first.  The minimum is kept as the maximum of 65536 - count,
// so that "none yet" is zero like everything else and one memset prepares the array.
struct KtrackAcc {
  uint64_t sum;
  uint32_t win, pres, solid, inv_min, mx, pad;
};
static_assert(sizeof(KtrackAcc) == 32, "two 16-byte halves");

struct KtrackArgs {
  const uint8_t *seqs;
  uint64_t nbytes;
  const uint64_t *offs;  // n + 1, checked
  uint32_t n;
  int k;
  uint32_t solid;  // max(min_count, 1)
  const uint32_t *index;
  uint64_t mask;
  const uint64_t *keys;
  const uint16_t *counts;
  uint16_t *track;  // nullptr: none
  KtrackAcc *acc;  // per sequence, zeroed; nullptr where neither records nor means are asked for
  uint16_t *mean;  // per sequence (FILL)
  uint4 *recs;     // kc_kdepth_rec, nullptr: none
  uint64_t *st;
};

__global__ void __launch_bounds__(KT_TPB) kc_ktrack_offsets_kernel(const uint64_t *offs, uint64_t n, uint64_t nbytes, uint64_t *st) {
  const uint64_t i = (uint64_t)blockIdx.x * KT_TPB + threadIdx.x;
  uint64_t len = 0;
  if (i < n) {
    const uint64_t a = offs[i], b = offs[i + 1];
    if (b < a)
      atomicMin((unsigned long long *)&st[KTS_BAD], (unsigned long long)i);
    else if (b - a >= (1ull << 32))
      atomicMin((unsigned long long *)&st[KTS_LONG], (unsigned long long)i);
    else
      len = b - a;
    if (i == 0 && a != 0) atomicOr((unsigned long long *)&st[KTS_ENDS], 1ull);
    if (i == n - 1 && b != nbytes) atomicOr((unsigned long long *)&st[KTS_ENDS], 2ull);
  }
  len = wave_max(len);
  if ((threadIdx.x & 63) == 0 && len) atomicMax((unsigned long long *)&st[KTS_LONGEST], (unsigned long long)len);
}

// what a lane has summed over windows of one sequence
struct KtrackSums {
  uint32_t sum, win, pres, solid, mn, mx;
  __device__ __forceinline__ void clear() { sum = win = pres = solid = mx = 0u, mn = 0xFFFFFFFFu; }
  __device__ __forceinline__ void add(uint32_t c, uint32_t solid_min) {
    win++;
    sum += c;
    if (c) {
      pres++;
      mn = c < mn ? c : mn;
      mx = c > mx ? c : mx;
    }
    solid += c >= solid_min;
  }
};

__device__ __forceinline__ void ktrack_flush(const KtrackArgs &a, uint32_t s, const KtrackSums &v) {
  if (!v.win) return;
  KtrackAcc *t = a.acc + s;
  atomicAdd(&t->win, v.win);
  if (!v.pres) return;
  atomicAdd((unsigned long long *)&t->sum, (unsigned long long)v.sum);
  atomicAdd(&t->pres, v.pres);
  if (v.solid) atomicAdd(&t->solid, v.solid);
  atomicMax(&t->inv_min, 65536u - v.mn);
  atomicMax(&t->mx, v.mx);
}

// The rest of kc_index_find's walk for a key whose home slot s held another key: from the slot behind it.
template <int NL>
__device__ __forceinline__ uint32_t ktrack_find_behind(const uint64_t (&f)[NL], uint64_t s, const uint32_t *index, uint64_t mask, const uint64_t *keys) {
  for (;;) {
    s = (s + 1) & mask;
    const uint32_t e = index[s];
    if (!e) return 0u;
    bool same = true;
#pragma unroll
    for (int j = 0; j < NL; j++) same &= keys[(uint64_t)(e - 1) * NL + j] == f[j];
    if (same) return e;
  }
}

template <int NL, bool FILL>
__global__ void __launch_bounds__(KT_TPB) kc_ktrack_windows_kernel(const KtrackArgs a) {
  const uint64_t p0 = ((uint64_t)blockIdx.x * KT_TPB + threadIdx.x) * KT_RUN;
  const bool live = p0 < a.nbytes;
  const int k = a.k, lw = (k - 1) >> 5, sh = 62 - 2 * ((k - 1) & 31);
  uint64_t f[NL], r[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) f[j] = r[j] = 0;
  uint32_t cur = 0, run = 0;
  uint64_t cur_end = 0;
  if (live) {
    cur = find_le(a.offs, 0u, a.n - 1u, p0);
    cur_end = a.offs[cur + 1];
  }
  KtrackSums acc;
  acc.clear();
  uint32_t acc_seq = 0;
  uint32_t t_win = 0, t_pres = 0, t_solid = 0, t_sum = 0;
  const int steps = live ? KT_RUN + k - 1 : 0;  // bytes p0 .. p0 + KT_RUN + k - 2; step t ends the window of position p0 + t - (k - 1)
  // one byte: the sequence it lies in, the run of bases it ends, the two words rolled on by it
  auto take = [&](uint64_t q, uint32_t byte) {
    while (q < a.nbytes && q >= cur_end) {  // a sequence starts here (empty ones are passed over)
      cur++;
      cur_end = a.offs[cur + 1];
      run = 0;
    }
    const uint32_t code = base_code4(byte);
    if (code < 4u) {
      run++;
#pragma unroll
      for (int j = 0; j < NL; j++) {
        f[j] = (f[j] << 2) | (j + 1 < NL ? f[j + 1] >> 62 : 0ULL);
        if (j == lw) f[j] |= (uint64_t)code << sh;
      }
#pragma unroll
      for (int j = NL - 1; j >= 0; j--) r[j] = ((r[j] >> 2) | (j ? r[j - 1] << 62 : (uint64_t)(3u - code) << 62)) & kc_word_mask(k, j);
    } else {
      run = 0;
    }
  };
  // the steps in front of the first group that can end a window only roll
  const int warm = live ? (k - 1) / KT_FLIGHT * KT_FLIGHT : 0;
  for (int t0 = 0; t0 < warm; t0 += KT_FLIGHT) {
    uint32_t byte[KT_FLIGHT];
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) {
      const uint64_t q = p0 + (uint32_t)(t0 + b);
      byte[b] = q < a.nbytes ? a.seqs[q] : 0u;
    }
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) take(p0 + (uint32_t)(t0 + b), byte[b]);
  }
  for (int t0 = warm; t0 < steps; t0 += KT_FLIGHT) {
    uint32_t byte[KT_FLIGHT];
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) {
      const uint64_t q = p0 + (uint32_t)(t0 + b);
      byte[b] = q < a.nbytes ? a.seqs[q] : 0u;
    }
    uint64_t key[KT_FLIGHT][NL], slot[KT_FLIGHT];
    uint32_t seq[KT_FLIGHT];
    bool win[KT_FLIGHT];
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) {
      take(p0 + (uint32_t)(t0 + b), byte[b]);
      win[b] = run >= (uint32_t)k && t0 + b < steps;
      seq[b] = cur;
      const bool fwd = !kc_less<NL>(r, f);
#pragma unroll
      for (int j = 0; j < NL; j++) key[b][j] = fwd ? f[j] : r[j];
      slot[b] = kc_hash<NL>(key[b]) & a.mask;
    }
    // ---- the probes of the windows among them, load by load
    uint32_t e[KT_FLIGHT];
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) e[b] = win[b] ? a.index[slot[b]] : 0u;
    bool other[KT_FLIGHT];
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) {
      other[b] = false;
      if (e[b]) {
        bool same = true;
#pragma unroll
        for (int j = 0; j < NL; j++) same &= a.keys[(uint64_t)(e[b] - 1) * NL + j] == key[b][j];
        other[b] = !same;
      }
    }
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++)
      if (other[b]) e[b] = ktrack_find_behind<NL>(key[b], slot[b], a.index, a.mask, a.keys);
    uint32_t cnt[KT_FLIGHT];
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) cnt[b] = e[b] ? (uint32_t)a.counts[e[b] - 1] : 0u;
#pragma unroll
    for (int b = 0; b < KT_FLIGHT; b++) {
      const int t = t0 + b;
      if (!FILL && a.track && t >= k - 1 && t < steps) {
        const uint64_t p = p0 + (uint32_t)(t - (k - 1));
        if (p < a.nbytes) a.track[p] = (uint16_t)cnt[b];
      }
      if (win[b]) {
        t_win++;
        t_pres += cnt[b] != 0u;
        t_solid += cnt[b] >= a.solid;
        t_sum += cnt[b];
        if (a.acc) {
          if (seq[b] != acc_seq) {
            ktrack_flush(a, acc_seq, acc);
            acc.clear();
            acc_seq = seq[b];
          }
          acc.add(cnt[b], a.solid);
        }
      }
    }
  }
  if (a.acc) {
    // a wave whose windows all lie in one sequence adds once; lanes without a window hold the neutral values
    const unsigned long long has = __ballot(acc.win != 0u);
    if (has) {
      const uint32_t s0 = (uint32_t)__shfl((int)acc_seq, __ffsll((long long)has) - 1);
      if (__all(!acc.win || acc_seq == s0)) {
        KtrackSums w;
        w.sum = wave_sum(acc.sum);
        w.win = wave_sum(acc.win);
        w.pres = wave_sum(acc.pres);
        w.solid = wave_sum(acc.solid);
        w.mn = wave_min(acc.mn);
        w.mx = wave_max(acc.mx);
        if ((threadIdx.x & 63) == 0) ktrack_flush(a, s0, w);
      } else {
        ktrack_flush(a, acc_seq, acc);
      }
    }
  }
  wg_stats(a.st, {KTS_WINDOWS, KTS_PRESENT, KTS_SOLID, KTS_SUM}, {t_win, t_pres, t_solid, t_sum});
}

// kc_kdepth_rec: {sum, windows, present}, {solid, min_count | max_count << 16, mean, 0}
__global__ void __launch_bounds__(KT_TPB) kc_ktrack_records_kernel(const KtrackArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * KT_TPB + threadIdx.x;
  if (i >= a.n) return;
  const KtrackAcc t = a.acc[i];
  const uint64_t sum = t.sum;
  const uint32_t win = t.win, pres = t.pres;
  const uint32_t mn = pres ? 65536u - t.inv_min : 0u, mx = t.mx;
  uint64_t mean = 0;
  if (win) {
    mean = (2 * sum + win) / (2 * (uint64_t)win);
    mean = mean > 65535u ? 65535u : mean;
  }
  if (a.mean) a.mean[i] = (uint16_t)mean;
  if (a.recs) {
    a.recs[2 * i] = make_uint4((uint32_t)sum, (uint32_t)(sum >> 32), win, pres);
    a.recs[2 * i + 1] = make_uint4(t.solid, mn | (mx << 16), (uint32_t)mean, 0u);
  }
}

__global__ void __launch_bounds__(KT_TPB) kc_ktrack_fill_kernel(const KtrackArgs a) {
  const uint64_t p0 = ((uint64_t)blockIdx.x * KT_TPB + threadIdx.x) * KT_FILL_ITEMS;
  if (p0 >= a.nbytes) return;
  uint32_t cur = find_le(a.offs, 0u, a.n - 1u, p0);
  uint64_t cur_end = a.offs[cur + 1];
  uint32_t mean = a.mean[cur];
  uint32_t v[KT_FILL_ITEMS];
#pragma unroll
  for (int j = 0; j < KT_FILL_ITEMS; j++) {
    const uint64_t p = p0 + j;
    v[j] = 0;
    if (p < a.nbytes) {
      while (p >= cur_end) {
        cur++;
        cur_end = a.offs[cur + 1];
        mean = a.mean[cur];
      }
      v[j] = base_code4(a.seqs[p]) < 4u ? mean : 0u;
    }
  }
  if (p0 + KT_FILL_ITEMS <= a.nbytes && (((uintptr_t)a.track) & 15) == 0) {
    *(uint4 *)(a.track + p0) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
  } else {
#pragma unroll
    for (int j = 0; j < KT_FILL_ITEMS; j++)
      if (p0 + j < a.nbytes) a.track[p0 + j] = (uint16_t)v[j];
  }
}

// ---- the count spectrum ------------------------------------------------------------------------------------------------
constexpr int SPECT_BINS = 65536;
constexpr int SPECT_LOW = 1024;  // bins a workgroup keeps in LDS
#ifndef KC_SPECT_REP
#define KC_SPECT_REP 4
#endif
constexpr int SPECT_REP = KC_SPECT_REP;  // copies of them
constexpr int SPECT_TPB = 256;
constexpr int SPECT_ITEMS = 8;  // counts a lane loads at once: 16 bytes
enum { SPS_KMERS = 0, SPS_SUM, SPS_MAX, SPS_MODE, SPS_MODE_KMERS, SPS_SATURATED, SPS_COUNT = 8 };

__device__ __forceinline__ void spect_add(uint32_t *sub, uint64_t *hist, uint32_t c, uint32_t rep) {
  if (c < (uint32_t)SPECT_LOW)
    atomicAdd(&sub[c * SPECT_REP + rep], 1u);
  else
    atomicAdd((unsigned long long *)&hist[c], 1ull);
}

// counts: 16-byte aligned (the results' own array); a workgroup sees fewer than 2^32 of them
__global__ void __launch_bounds__(SPECT_TPB) kc_spect_hist_kernel(const uint16_t *counts, uint64_t n, uint64_t *hist) {
  __shared__ uint32_t sub[SPECT_LOW * SPECT_REP];
  for (int j = threadIdx.x; j < SPECT_LOW * SPECT_REP; j += SPECT_TPB) sub[j] = 0u;
  __syncthreads();
  const uint32_t rep = threadIdx.x % SPECT_REP;
  const uint64_t stride = (uint64_t)gridDim.x * SPECT_TPB * SPECT_ITEMS;
  for (uint64_t i = ((uint64_t)blockIdx.x * SPECT_TPB + threadIdx.x) * SPECT_ITEMS; i < n; i += stride) {
    if (i + SPECT_ITEMS <= n) {
      const uint4 v = *(const uint4 *)(counts + i);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        spect_add(sub, hist, w[j] & 0xFFFFu, rep);
        spect_add(sub, hist, w[j] >> 16, rep);
      }
    } else {
      for (uint64_t j = i; j < n; j++) spect_add(sub, hist, counts[j], rep);
    }
  }
  __syncthreads();
  for (int bin = threadIdx.x; bin < SPECT_LOW; bin += SPECT_TPB) {
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < SPECT_REP; j++) s += sub[bin * SPECT_REP + j];
    if (s) atomicAdd((unsigned long long *)&hist[bin], (unsigned long long)s);
  }
}

// the greater number of k-mers, the smaller count among equals
struct SpectMode {
  uint64_t kmers;
  uint32_t count;
  __device__ __forceinline__ SpectMode across(int o) const { return {__shfl_xor(kmers, o), __shfl_xor(count, o)}; }
  __device__ __forceinline__ SpectMode join(const SpectMode &b) const {
    return (b.kmers > kmers || (b.kmers == kmers && b.count < count)) ? b : *this;
  }
};

__global__ void __launch_bounds__(1024) kc_spect_stats_kernel(const uint64_t *hist, uint64_t *st) {
  __shared__ uint64_t s_kmers[16], s_sum[16], s_mode_kmers[16];
  __shared__ uint32_t s_max[16], s_mode[16];
  uint64_t kmers = 0, sum = 0;
  uint32_t mx = 0;
  SpectMode mode{0, 0};
  for (uint32_t c = threadIdx.x; c < (uint32_t)SPECT_BINS; c += 1024) {
    const uint64_t h = hist[c];
    kmers += h;
    sum += h * c;
    if (h) mx = c;  // c rises
    mode = mode.join(SpectMode{h, c});
  }
  kmers = wave_sum(kmers);
  sum = wave_sum(sum);
  mx = wave_max(mx);
  mode = wave_join(mode);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_kmers[w] = kmers, s_sum[w] = sum, s_max[w] = mx, s_mode[w] = mode.count, s_mode_kmers[w] = mode.kmers;
  __syncthreads();
  if (threadIdx.x == 0) {
    kmers = sum = 0, mx = 0, mode = SpectMode{0, 0};
    for (int j = 0; j < 16; j++) {
      kmers += s_kmers[j];
      sum += s_sum[j];
      mx = s_max[j] > mx ? s_max[j] : mx;
      mode = mode.join(SpectMode{s_mode_kmers[j], s_mode[j]});
    }
    st[SPS_KMERS] = kmers;
    st[SPS_SUM] = sum;
    st[SPS_MAX] = mx;
    st[SPS_MODE] = mode.kmers ? mode.count : 0;
    st[SPS_MODE_KMERS] = mode.kmers;
    st[SPS_SATURATED] = hist[SPECT_BINS - 1];
    st[6] = st[7] = 0;
  }
}

}  // namespace kc
