// kc_correct.hpp -- read correction from the finished results (kc_correct_reads).  DESIGN.md section 32 holds the rules; they
// are this project's own, pinned by the host model tests/correct_model.py.  A round is: the depth track of the current text
// (kc_ktrack_windows_kernel<NL, false> of kc_kdepth.hpp, as it stands), the sites, their evaluation, the accepted bytes.
//
//  kc_correct_sites_kernel<WRITE>  a lane owns KT_RUN positions of the track and looks one further on either side.  A position
//                                  is solid (count >= S), weak (a window below S) or no window; a count of 0 says neither
//                                  "absent" nor "no window", so a lane that holds one rolls the bytes once, as the track
//                                  kernel does.  The position before a sequence's first is never a window (k >= 2), so runs
//                                  need no sequence test.  A lane that owns a run's first or last position walks at most 2k
//                                  track values from an anchored end and decides the site; from an open first position it
//                                  walks to the run's end, whatever its length, to tell UNANCHORED from "anchored on the
//                                  right".  The count pass leaves a count per lane and per workgroup, the weak windows and
//                                  the reasons per sequence; after the scan of the workgroups' counts the write pass puts
//                                  the sites down in (seq, pos) order.
//  kc_correct_eval_kernel<NL>      a wave per site.  The n + k - 1 bytes under the range's windows go to LDS as 2-bit codes in
//                                  the key's bit order; a lane cuts the window of its (alternative, window) pair out with two
//                                  64-bit loads and a funnel shift a word, patches the site's base, forms the canonical key
//                                  and probes the index.  A ballot gathers the solid bits in range order, the trailing ones
//                                  of an alternative's part are its score; lane 0 writes the verdict.
//  kc_correct_apply_kernel         a thread per site: an accepted one writes its byte and its fix entry, at the slot the scan
//                                  of the accept flags gave it.
//  kc_correct_records_kernel       a thread per sequence: kc_correct_rec.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_kdepth.hpp"

namespace kc {

constexpr int CR_TPB = 256;
constexpr int CR_WAVES = CR_TPB / 64;
constexpr int CR_WORDS = 16;  // 64-bit words of 2-bit codes a wave keeps: n + k - 1 <= 249 codes in 8, and NL + 1 beyond a window's first
enum { CRF_UNANCHORED = 1, CRF_SHORT_RUN = 2, CRF_THIN = 4, CRF_QUAL_GATED = 8, CRF_NO_GAIN = 16, CRF_AMBIGUOUS = 32 };
enum { CRC_NON = 0, CRC_WEAK, CRC_SOLID };

struct CorrectArgs {
  uint8_t *text;         // the current text: nbytes
  const uint8_t *quals;  // nullptr: no gate
  uint64_t nbytes;
  const uint64_t *offs;  // n + 1, checked
  uint32_t n;
  int k;
  uint32_t solid;  // max(min_count, 1)
  uint32_t min_gain, min_windows, max_qual;
  int qual_offset;
  const uint16_t *track;  // of the current text
  uint8_t *lane_sites;    // sites a lane of the sites kernel gives
  uint64_t *wg_sites;     // ... a workgroup; after the scan: where its first goes
  uint32_t *weak;         // per sequence: weak windows of the current text (zeroed)
  uint32_t *why_sites;    // per sequence: reasons of runs and dropped sites (zeroed); nullptr: not asked for
  uint32_t *why_eval;     // per sequence: reasons of evaluated sites (zeroed)
  uint32_t *corrected;    // per sequence: accepted sites of all rounds (zeroed once)
  uint32_t *weak_before;  // per sequence: `weak` of the first round
  uint4 *sites;           // {seq, pos, side | n << 8, 0}
  uint64_t n_sites;
  uint2 *verdicts;  // {accepted | y << 8, score | runner_up << 16}
  uint64_t *slots;  // the accept flags, then their exclusive scan
  uint4 *fixes;     // kc_correct_fix, this round's
  uint32_t round;   // from 1
  const uint32_t *index;
  uint64_t mask;
  const uint64_t *keys;
  const uint16_t *counts;
  uint4 *recs;  // kc_correct_rec
};

// the walk from a run's first position `a` towards its end: the number of weak windows, stopped at `most`, and what follows
// them.  Window a + j - 1 is known to be one, so window a + j is one iff its last byte is a base of the sequence.
__device__ __forceinline__ uint32_t correct_walk_up(const CorrectArgs &a, uint64_t at, uint64_t seq_end, uint32_t most, int &after) {
  uint32_t len = 1;
  after = CRC_WEAK;
  for (; len < most; len++) {
    const uint64_t q = at + len;
    if (q + (uint32_t)a.k > seq_end) {
      after = CRC_NON;
      break;
    }
    if (a.track[q] >= a.solid) {
      after = CRC_SOLID;
      break;
    }
    if (base_code4(a.text[q + (uint32_t)a.k - 1]) >= 4u) {
      after = CRC_NON;
      break;
    }
  }
  return len;
}

// ... from its last position `at` towards its start: window at - j + 1 is one, so window at - j is one iff its first byte is a base
__device__ __forceinline__ uint32_t correct_walk_down(const CorrectArgs &a, uint64_t at, uint64_t seq_start, uint32_t most, int &before) {
  uint32_t len = 1;
  before = CRC_WEAK;
  for (; len < most; len++) {
    if (at - seq_start < len) {
      before = CRC_NON;
      break;
    }
    const uint64_t q = at - len;
    if (a.track[q] >= a.solid) {
      before = CRC_SOLID;
      break;
    }
    if (base_code4(a.text[q]) >= 4u) {
      before = CRC_NON;
      break;
    }
  }
  return len;
}

template <bool WRITE>
__global__ void __launch_bounds__(CR_TPB) kc_correct_sites_kernel(const CorrectArgs a) {
  __shared__ uint32_t wave_sites[CR_WAVES];
  const uint64_t gid = (uint64_t)blockIdx.x * CR_TPB + threadIdx.x;
  const uint64_t p0 = gid * KT_RUN;
  const bool live = p0 < a.nbytes;
  const uint32_t k = (uint32_t)a.k;
  // bit i of the masks: position p0 - 1 + i, i = 0 .. KT_RUN + 1
  uint32_t solid = 0, nonzero = 0, valid = 0;
  if (live) {
#pragma unroll
    for (int i = 0; i < KT_RUN + 2; i++) {
      const bool ok = (i > 0 || p0 > 0) && p0 + (uint32_t)i - 1 < a.nbytes;
      const uint32_t v = ok ? a.track[p0 + (uint32_t)i - 1] : 0u;
      valid |= (uint32_t)ok << i;
      solid |= (uint32_t)(v >= a.solid) << i;
      nonzero |= (uint32_t)(v != 0u) << i;
    }
  }
  uint32_t window = nonzero;
  if (valid & ~nonzero) {  // a count of 0: absent, or no window
    const uint64_t q0 = p0 ? p0 - 1 : 0;
    const uint32_t bit0 = p0 ? 0u : 1u;
    uint32_t cur = find_le(a.offs, 0u, a.n - 1u, q0), run = 0;
    uint64_t cur_end = a.offs[cur + 1];
    const uint32_t steps = KT_RUN + 2 - bit0 + k - 1;
    for (uint32_t t = 0; t < steps; t++) {
      const uint64_t q = q0 + t;
      if (q >= a.nbytes) break;
      while (q >= cur_end) {
        cur++;
        cur_end = a.offs[cur + 1];
        run = 0;
      }
      run = base_code4(a.text[q]) < 4u ? run + 1 : 0u;
      if (run >= k) window |= 1u << (t - (k - 1) + bit0);
    }
  }
  const uint32_t weak = window & ~solid & valid;
  const uint32_t own = weak & (((1u << KT_RUN) - 1u) << 1);
  uint32_t n_sites = 0;
  uint64_t dst = 0;
  if (WRITE) {
    // where the lane's first site goes: the workgroup's base and the lanes in front of it
    const uint32_t mine = live ? a.lane_sites[gid] : 0u;
    uint32_t inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o);
      if ((int)(threadIdx.x & 63) >= o) inc += t;
    }
    if ((threadIdx.x & 63) == 63) wave_sites[threadIdx.x >> 6] = inc;
    __syncthreads();
    dst = a.wg_sites[blockIdx.x] + inc - mine;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) dst += wave_sites[w];
    if (!mine) return;
  }
  if (own) {
    uint32_t cur = 0, in_seq = 0, why = 0;
    uint64_t cur_start = 0, cur_end = 0;
    bool found = false;
    // a site of the run: dropped with its reason, counted, or written
    auto site = [&](uint32_t side, uint64_t e, uint32_t n) {
      if (n < a.min_windows) {
        why |= CRF_THIN;
      } else if (a.quals && a.max_qual && (int)a.quals[e] - a.qual_offset > (int)a.max_qual) {
        why |= CRF_QUAL_GATED;
      } else {
        if (WRITE) a.sites[dst + n_sites] = make_uint4(cur, (uint32_t)(e - cur_start), side | (n << 8), 0u);
        n_sites++;
      }
    };
    auto flush = [&]() {
      if (WRITE) return;
      if (in_seq) atomicAdd(&a.weak[cur], in_seq);
      if (why && a.why_sites) atomicOr(&a.why_sites[cur], why);
      in_seq = why = 0;
    };
    for (uint32_t i = 1; i <= (uint32_t)KT_RUN; i++) {
      if (!((own >> i) & 1u)) continue;
      const uint64_t p = p0 + i - 1;
      if (!found) {
        cur = find_le(a.offs, 0u, a.n - 1u, p);
        cur_start = a.offs[cur];
        cur_end = a.offs[cur + 1];
        found = true;
      }
      if (p >= cur_end) {
        flush();
        while (p >= cur_end) {
          cur++;
          cur_end = a.offs[cur + 1];
        }
        cur_start = a.offs[cur];
      }
      in_seq++;
      if (!((weak >> (i - 1)) & 1u)) {  // the run's first position
        if ((solid >> (i - 1)) & 1u) {
          int after;
          const uint32_t len = correct_walk_up(a, p, cur_end, 2 * k, after);
          if (len >= 2 * k || after != CRC_SOLID)
            site(0u, p + k - 1, len < k ? len : k);
          else if (len < k)
            why |= CRF_SHORT_RUN;
          else
            site(0u, p + k - 1, k);
        } else if (!WRITE && a.why_sites) {
          int after;
          (void)correct_walk_up(a, p, cur_end, 0xFFFFFFFFu, after);
          if (after != CRC_SOLID) why |= CRF_UNANCHORED;
        }
      }
      if (!((weak >> (i + 1)) & 1u) && ((solid >> (i + 1)) & 1u)) {  // the last position of a run anchored on the right
        int before;
        const uint32_t len = correct_walk_down(a, p, cur_start, 2 * k, before);
        if (len >= 2 * k || before != CRC_SOLID) site(1u, p, len < k ? len : k);
      }
    }
    flush();
  }
  if (!WRITE) {
    if (live) a.lane_sites[gid] = (uint8_t)n_sites;
    const uint32_t w = wave_sum(n_sites);
    if ((threadIdx.x & 63) == 0) wave_sites[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t s = 0;
      for (int j = 0; j < CR_WAVES; j++) s += wave_sites[j];
      a.wg_sites[blockIdx.x] = s;
    }
  }
}

// the trailing ones of `bits`, of which `len` (1 .. 64) count
__device__ __forceinline__ uint32_t correct_trailing_ones(uint64_t bits, uint32_t len) {
  const uint32_t t = (uint32_t)__ffsll((long long)~bits);  // 0: all 64 are ones
  const uint32_t ones = t ? t - 1 : 64u;
  return ones < len ? ones : len;
}

template <int NL>
__global__ void __launch_bounds__(CR_TPB) kc_correct_eval_kernel(const CorrectArgs a) {
  __shared__ uint64_t codes[CR_WAVES][CR_WORDS];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t s = (uint64_t)blockIdx.x * CR_WAVES + wv;
  const bool active = s < a.n_sites;  // the same for a whole wave
  const uint4 site = active ? a.sites[s] : make_uint4(0u, 0u, 1u << 8, 0u);
  const uint32_t k = (uint32_t)a.k, side = site.z & 0xFFu, n = site.z >> 8;
  const uint64_t e = active ? a.offs[site.x] + site.y : 0;
  const uint64_t lo = side ? e - (n - 1) : e - (k - 1);  // the first byte under the range's windows; n + k - 1 of them
  const uint32_t len = active ? n + k - 1 : 0u, e_at = (uint32_t)(e - lo);
  uint64_t *w = codes[wv];
  if (lane < (uint32_t)CR_WORDS) w[lane] = 0;
  __syncthreads();
  for (uint32_t j = lane; j < len; j += 64) {
    const uint64_t code = base_code4(a.text[lo + j]) & 3u;  // every byte of a window is a base
    atomicOr((unsigned long long *)&w[j >> 5], (unsigned long long)(code << (62 - 2 * (j & 31))));
  }
  __syncthreads();
  if (!active) return;
  const uint32_t x = (uint32_t)(w[e_at >> 5] >> (62 - 2 * (e_at & 31))) & 3u;
  uint32_t score[3] = {0, 0, 0};
  uint32_t open = 7u;
  for (uint32_t first = 0; first < 3 * n && open; first += 64) {
    const uint32_t pair = first + lane, alt = pair / n, r = pair - alt * n;  // r: the window's place in the range
    bool is_solid = false;
    if (pair < 3 * n && ((open >> alt) & 1u)) {
      const uint32_t o = side ? n - 1 - r : r;  // the window's first code
      const uint32_t at = e_at - o;             // the site's place in the window
      const uint32_t y = alt + (alt >= x);
      const uint32_t sh = 2 * (o & 31);
      uint64_t f[NL], rc[NL];
#pragma unroll
      for (int j = 0; j < NL; j++) {
        const uint64_t hi = w[(o >> 5) + j], lw = w[(o >> 5) + j + 1];
        f[j] = (sh ? (hi << sh) | (lw >> (64 - sh)) : hi) & kc_word_mask(a.k, j);
        if ((int)(at >> 5) == j) f[j] = (f[j] & ~(3ull << (62 - 2 * (at & 31)))) | ((uint64_t)y << (62 - 2 * (at & 31)));
      }
      kc_revcomp<NL>(f, a.k, rc);
      if (kc_less<NL>(rc, f)) {
#pragma unroll
        for (int j = 0; j < NL; j++) f[j] = rc[j];
      }
      const uint64_t slot = kc_hash<NL>(f) & a.mask;
      uint32_t en = a.index[slot];
      if (en) {
        bool same = true;
#pragma unroll
        for (int j = 0; j < NL; j++) same &= a.keys[(uint64_t)(en - 1) * NL + j] == f[j];
        if (!same) en = ktrack_find_behind<NL>(f, slot, a.index, a.mask, a.keys);
      }
      is_solid = en && a.counts[en - 1] >= a.solid;
    }
    const uint64_t got = __ballot(is_solid);
#pragma unroll
    for (uint32_t t = 0; t < 3; t++) {
      // the pairs of alternative t among this trip's: [from, to)
      const uint32_t from = t * n > first ? t * n : first, to = (t + 1) * n < first + 64 ? (t + 1) * n : first + 64;
      if (from < to && ((open >> t) & 1u)) {
        const uint32_t ones = correct_trailing_ones(got >> (from - first), to - from);
        score[t] += ones;
        if (ones < to - from) open &= ~(1u << t);
      }
    }
  }
  if (lane == 0) {
    const uint32_t need = n < a.min_gain ? n : a.min_gain;
    const uint32_t s0 = score[0], s1 = score[1], s2 = score[2];
    const uint32_t best = s0 >= s1 ? (s0 >= s2 ? 0u : 2u) : (s1 >= s2 ? 1u : 2u);
    const uint32_t top = best == 0 ? s0 : best == 1 ? s1 : s2;
    const uint32_t ra = best == 0 ? s1 : s0, rb = best == 2 ? s1 : s2;  // the other two
    const uint32_t runner = ra > rb ? ra : rb;
    const bool accept = top >= need && top > runner;
    if (!accept) atomicOr(&a.why_eval[site.x], top >= need ? (uint32_t)CRF_AMBIGUOUS : (uint32_t)CRF_NO_GAIN);
    a.verdicts[s] = make_uint2((uint32_t)accept | ((best + (best >= x)) << 8), top | (runner << 16));
    a.slots[s] = accept;
  }
}

__global__ void __launch_bounds__(CR_TPB) kc_correct_apply_kernel(const CorrectArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * CR_TPB + threadIdx.x;
  if (s >= a.n_sites) return;
  const uint2 v = a.verdicts[s];
  if (!(v.x & 1u)) return;
  const uint4 site = a.sites[s];
  const uint64_t e = a.offs[site.x] + site.y;
  const uint32_t old = a.text[e], now = code_letter(v.x >> 8) | (old & 0x20u);
  a.text[e] = (uint8_t)now;
  a.fixes[a.slots[s]] = make_uint4(site.x, site.y, old | (now << 8) | (a.round << 16) | ((site.z & 0xFFu) << 24), v.y);
  atomicAdd(&a.corrected[site.x], 1u);
}

// kc_correct_rec: weak_before, weak_after, corrected | flags << 16, 0
__global__ void __launch_bounds__(CR_TPB) kc_correct_records_kernel(const CorrectArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * CR_TPB + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t c = a.corrected[i];
  a.recs[i] = make_uint4(a.weak_before[i], a.weak[i], (c > 65535u ? 65535u : c) | ((a.why_sites[i] | a.why_eval[i]) << 16), 0u);
}

}  // namespace kc
