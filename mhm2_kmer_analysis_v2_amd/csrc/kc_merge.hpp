// kc_merge.hpp -- overlap merge of read pairs on the device (kc_merge_pairs): the pair loop of the reference's
// merge_reads (src/merge_reads.cpp:469-648) with no adapter file (Adapters::trim_pair returns at once when
// adapter_seqs is empty, src/adapters.cpp:260-261), producing the read cache's packed bytes.
// With an adapter file that step is kc_trim_adapters (kc_trim.hpp), run in front of this one.
//
// Rules (the contract of the kernels below and of tests/merge_model.py):
//  * Input: interleaved mates in one set of arrays, ASCII bases and qualities, offsets of 2*npairs+1 entries; read 2p
//    is mate 1, read 2p+1 mate 2 (the layout of kc_submit_reads).
//  * A pair is dropped (no output) when both mates are shorter than min_kmer_len (:473).
//  * len = min(len1, len2), start_i = len1 - len (:486-487); trials i = 0 .. len - MIN_OVERLAP + EXTRA_TEST_OVERLAP - 1
//    (:494) with MIN_OVERLAP 12, EXTRA_TEST_OVERLAP 2, MAX_MISMATCHES 3, EXTRA_MISMATCHES_PER_1000 150,
//    MAX_PERROR 0.025, MAX_MATCH_QUAL 41 (:344-354).  overlap = len - i, this_max_mismatch = 3 + 150 * overlap / 1000,
//    error_max_mismatch = this_max_mismatch * 4 / 3 + 1 (:496-498), all integer arithmetic.
//  * A trial whose byte mismatch count over the overlap exceeds error_max_mismatch is skipped (fast_count_mismatches,
//    :195-236, :499-500).  Otherwise the exact loop runs (:501-568): an N against a non-N counts two mismatches; two
//    matched Ns abort the pair (bothNs, :510-514), so does Ncount > 3 (:562-566), each adding one to num_ambiguous;
//    the loop breaks once mismatches > error_max_mismatch (:567).  perror is a double summed in position order over
//    the Q2Perror table (kc_q2perror below, :74-82): an N adds the other side's Q2Perror, every mismatch adds 0.5 when
//    the two qualities differ by at most 2 and Q2Perror[diff] otherwise, the N side's quality counting as 0.
//  * Resolution in offset order (:569-597): a good trial (matches >= max(overlap - this_max_mismatch, 12), the whole
//    overlap checked, mismatches <= this_max_mismatch, perror / overlap <= 0.025) becomes best_i if neither a best nor a
//    weak trial came before, else it is ambiguous and the loop stops; a weak trial (whole overlap, mismatches <=
//    error_max_mismatch, perror / overlap <= 0.025 * 4 / 3) sets found_i and, after a best_i, is ambiguous and stops the
//    loop.  An abort stops the loop after its own trial is resolved.  A pair merges when best_i >= 0 and nothing
//    aborted (:600).
//  * Bytes: mate 2 is reverse-complemented by revcomp (src/utils.cpp:98-129): IUPAC -> N, lower case -> upper case.
//    Mate 1 is compared byte by byte as it came, so a lower-case or IUPAC base of mate 1 equals nothing (and a lower-case
//    n is no N).  A byte outside kc_fastq_to_packed's table is KC_ERR_BAD_BASE.  A quality outside
//    [qual_offset, qual_offset + 80] or a mate longer than 32767 is KC_ERR_INVALID_ARG: stricter than the reference,
//    which asserts or DIEs only where it meets one (:524-545, fast_count_mismatches' assert).
//  * Side effects: a trial writes qual_offset into quals1 at an N of mate 1 that it compares with a non-N (:521), and
//    into rev_quals2 at an N of the reversed mate 2 compared with a non-N (:529).  The writes persist across trials, into
//    the merge and into an unmerged mate 1's output.  Every executed trial writes, those after best_i included, until
//    the loop stops.  No trial's outcome depends on them: the side written is always the N side, whose quality the
//    trial takes as 0 anyway.  So the decision is made without them, and a pair holding an N replays its executed
//    trials (those up to the stop offset that pass the prefilter) to apply them before it is written.
//  * Merge (:600-630): a match gets min(q1 + q2, 41), a mismatch the higher-quality base (mate 1's on a tie) and
//    max(|q1 - q2|, 2) (qualities relative to qual_offset); then the tail of the reversed mate 2 with its qualities.
//  * Output: the read cache's bytes, code | min(q, 31) << 3 (kc_fastq_to_packed's table), in pair order: one read for a
//    merged pair, both mates as they came (mate 2 not reverse-complemented) for an unmerged pair, nothing for a dropped
//    one.  The dummy one-base "N" mate the reference adds after a merged pair (:627) holds no k-mer and is not produced.
//
// Kernels (one decision pass, one scan, one write pass):
//  kc_merge_decide_kernel  a workgroup takes MG_TILE pairs, a wave one pair at a time.  The mates go to LDS (mate 1
//                          as it came, mate 2 reverse-complemented, qualities relative); lane l takes the trial offsets
//                          l, l + 64, ...: the prefilter counts differing bytes four at a time (aligned words of the
//                          reversed mate against funnel-shifted words of mate 1), the few offsets that pass run the
//                          exact loop, and a ballot of the trials that decide something resolves them in offset order.
//                          Stores a per-pair decision and size, per-tile sums and the statistics.  A pair with a mate
//                          longer than MG_MAXL goes to a list instead ...
//  <long>                  ... served by the same code, one wave per workgroup and the pair's bytes in dynamic LDS.
//  kc_scan_kernel<2>       (kc_scan.hpp) one workgroup: exclusive scan of the per-tile bytes and reads, the totals.
//  kc_merge_write_kernel   a workgroup per tile: in-tile offsets, the pair to LDS again, the replay for pairs with an
//                          N, then the packed bytes and the read offsets (and <long> for the listed pairs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_common.hpp"
#include "kc_scan.hpp"

namespace kc {

constexpr int MG_MIN_OVERLAP = 12;      // merge_reads.cpp:344
constexpr int MG_EXTRA_TEST_OVERLAP = 2;
constexpr int MG_MAX_MISMATCHES = 3;
constexpr int MG_EXTRA_PER_1000 = 150;  // :353
constexpr int MG_MAX_MATCH_QUAL = 41;   // :354, relative to qual_offset
constexpr int MG_MAX_QUAL = 80;         // Q2Perror has 81 entries
constexpr int MG_MAX_LEN = 32767;       // int16_t lengths of the pair loop
constexpr int MG_MAXL = 512;            // mates up to this long are served from static LDS
constexpr int MG_PAD = 8;               // LDS bytes behind a mate: the prefilter's funnel reads one word past the end
constexpr int MG_WAVES = 4;
constexpr int MG_TILE = 64;             // pairs per workgroup of the tiled kernels
constexpr int MG_SLOTS = 64;            // spread of the statistics counters

enum { MGS_MERGED = 0, MGS_AMBIG, MGS_DROPPED, MGS_OVERLAP, MGS_MERGED_LEN, MGS_N };
enum { MG_CTL_ERR = 0, MG_CTL_NLONG, MG_CTL_LONGMAX, MG_CTL_N };
enum { MG_ERR_BASE = 1, MG_ERR_ARG = 2 };
// pair decision word: bits 0..15 best_i + 2 (0 dropped, 1 unmerged), bit 16 replay (an N), bit 17 long
constexpr uint32_t MG_DEC_REPLAY = 1u << 16;
constexpr uint32_t MG_DEC_LONG = 1u << 17;

// Q2Perror, src/merge_reads.cpp:74-82 (data that decides borderline merges: kept digit for digit)
__constant__ double kc_q2perror[81] = {
    1.0,       0.7943,    0.6309,    0.5012,    0.3981,    0.3162,    0.2512,    0.1995,    0.1585,    0.1259,     0.1,
    0.07943,   0.06310,   0.05012,   0.03981,   0.03162,   0.02512,   0.01995,   0.01585,   0.01259,   0.01,       0.007943,
    0.006310,  0.005012,  0.003981,  0.003162,  0.002512,  0.001995,  0.001585,  0.001259,  0.001,     0.0007943,  0.0006310,
    0.0005012, 0.0003981, 0.0003162, 0.0002512, 0.0001995, 0.0001585, 0.0001259, 0.0001,    7.943e-05, 6.310e-05,  5.012e-05,
    3.981e-05, 3.162e-05, 2.512e-05, 1.995e-05, 1.585e-05, 1.259e-05, 1e-05,     7.943e-06, 6.310e-06, 5.012e-06,  3.981e-06,
    3.162e-06, 2.512e-06, 1.995e-06, 1.585e-06, 1.259e-06, 1e-06,     7.943e-07, 6.310e-07, 5.012e-07, 3.981e-07,  3.1622e-07,
    2.512e-07, 1.995e-07, 1.585e-07, 1.259e-07, 1e-07,     7.943e-08, 6.310e-08, 5.012e-08, 3.981e-08, 3.1622e-08, 2.512e-08,
    1.995e-08, 1.585e-08, 1.259e-08, 1e-08};

struct MergeArgs {
  const uint8_t *bases, *quals;
  const uint64_t *offsets;
  uint64_t npairs;
  int qoff, min_len;
  uint32_t *pair_dec;    // [npairs] decision word
  uint32_t *pair_out;    // [npairs] output bytes << 2 | output reads
  uint32_t *long_list;   // [npairs] pairs with a mate longer than MG_MAXL
  uint64_t *tile_bytes;  // [ntiles] sums, then (kc_scan_kernel) exclusive bases
  uint64_t *tile_reads;
  uint64_t *totals;      // [2] bytes, reads
  uint64_t *stats;       // [MG_SLOTS][MGS_N]
  uint32_t *ctl;         // [MG_CTL_N]
  uint8_t *out;          // packed bytes
  uint64_t *out_offsets; // [reads + 1]
};

// kc_fastq_to_packed's table (PackedRead, src/packed_reads.cpp:99-124): ACGT/acgt 0..3, N n and upper-case IUPAC 4,
// anything else 255.  Every accepted byte lies in [64, 128): one bit mask per class instead of a switch (a switch on a
// per-lane byte is a chain of divergent branches).
constexpr uint64_t mg_bits(const char *s) { return *s ? (1ull << ((uint32_t)*s & 63u)) | mg_bits(s + 1) : 0ull; }
constexpr uint64_t MG_ACGT = mg_bits("ACGTacgt");
constexpr uint64_t MG_FOUR = mg_bits("NnURYKMSWBDHV");

__device__ __forceinline__ uint32_t mg_code(uint32_t c) {
  const bool hi = (c >> 6) == 1u;
  if (hi && ((MG_ACGT >> (c & 63u)) & 1u)) return kc_base_code(c);
  return hi && ((MG_FOUR >> (c & 63u)) & 1u) ? 4u : 255u;
}

// revcomp's complement (src/utils.cpp:101-126) of a byte mg_code accepts: acgt/ACGT -> TGCA, the rest -> N
__device__ __forceinline__ uint32_t mg_comp(uint32_t c) {
  const bool acgt = (c >> 6) == 1u && ((MG_ACGT >> (c & 63u)) & 1u);
  return acgt ? (0x41434754u >> (8u * kc_base_code(c))) & 0xFFu : (uint32_t)'N';
}

__device__ __forceinline__ void mg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// one wave's view of a pair in LDS
struct MgBufs {
  uint8_t *s1, *q1, *rc, *rq;  // mate 1, its qualities, reversed-complemented mate 2, its reversed qualities
  const double *pe;            // Q2Perror in LDS (a divergent index into __constant__ memory is a vector load)
};

__device__ __forceinline__ MgBufs mg_bufs(uint8_t *lds, int cap, const double *pe) {
  const int stride = cap + MG_PAD;
  return MgBufs{lds, lds + stride, lds + 2 * stride, lds + 3 * stride, pe};
}

__device__ __forceinline__ void mg_load_table(double *pe) {
  for (int t = threadIdx.x; t < 81; t += blockDim.x) pe[t] = kc_q2perror[t];
  __syncthreads();
}

// the pair's mates: global offsets and lengths; false (and an error flag) for a length the pair loop cannot take
__device__ __forceinline__ bool mg_pair(const MergeArgs &a, uint64_t p, uint64_t &o1, uint64_t &o2, int &len1, int &len2) {
  o1 = a.offsets[2 * p];
  o2 = a.offsets[2 * p + 1];
  const uint64_t e2 = a.offsets[2 * p + 2];
  const uint64_t l1 = o2 - o1, l2 = e2 - o2;
  if (l1 > (uint64_t)MG_MAX_LEN || l2 > (uint64_t)MG_MAX_LEN) return false;
  len1 = (int)l1;
  len2 = (int)l2;
  return true;
}

// the mates into LDS (relative qualities); returns error flags (wave-uniform) and whether either mate holds an 'N'.
// FAST (mates of at most MG_MAXL bases): every load of the pair is issued before the first store, one round trip.
template <bool FAST>
__device__ __forceinline__ uint32_t mg_load(const MergeArgs &a, const MgBufs &b, uint64_t o1, uint64_t o2, int len1, int len2, int lane,
                                            bool &anyN) {
  uint32_t err = 0;
  bool n = false;
  auto put = [&](int t, uint32_t c1, int q1, uint32_t c2, int q2) {
    if (t < len1) {
      if (mg_code(c1) == 255) err |= MG_ERR_BASE;
      if (q1 < 0 || q1 > MG_MAX_QUAL) err |= MG_ERR_ARG;
      n |= c1 == 'N';
      b.s1[t] = (uint8_t)c1;
      b.q1[t] = (uint8_t)q1;
    }
    if (t < len2) {
      if (mg_code(c2) == 255) err |= MG_ERR_BASE;
      if (q2 < 0 || q2 > MG_MAX_QUAL) err |= MG_ERR_ARG;
      const uint32_t r = mg_comp(c2);
      n |= r == 'N';
      b.rc[t] = (uint8_t)r;
      b.rq[t] = (uint8_t)q2;
    }
  };
  if (FAST) {
    constexpr int K = MG_MAXL / 64;
    uint32_t c1[K], c2[K], q1[K], q2[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int t = lane + 64 * k;
      c1[k] = t < len1 ? a.bases[o1 + t] : 0u;
      q1[k] = t < len1 ? a.quals[o1 + t] : 0u;
      c2[k] = t < len2 ? a.bases[o2 + len2 - 1 - t] : 0u;
      q2[k] = t < len2 ? a.quals[o2 + len2 - 1 - t] : 0u;
    }
#pragma unroll
    for (int k = 0; k < K; k++) put(lane + 64 * k, c1[k], (int)q1[k] - a.qoff, c2[k], (int)q2[k] - a.qoff);
  } else {
    const int m = len1 > len2 ? len1 : len2;
    for (int t = lane; t < m; t += 64) {
      const uint32_t c1 = t < len1 ? a.bases[o1 + t] : 0u, q1 = t < len1 ? a.quals[o1 + t] : 0u;
      const uint32_t c2 = t < len2 ? a.bases[o2 + len2 - 1 - t] : 0u, q2 = t < len2 ? a.quals[o2 + len2 - 1 - t] : 0u;
      put(t, c1, (int)q1 - a.qoff, c2, (int)q2 - a.qoff);
    }
  }
  mg_wave_sync();
  anyN = __ballot(n) != 0;
  uint32_t e = err;
  for (int s = 1; s < 64; s <<= 1) e |= __shfl_xor(e, s);
  return e;
}

// bytes of x that are not zero
__device__ __forceinline__ int mg_nonzero_bytes(uint32_t x) {
  uint32_t t = x | (x >> 4);
  t |= t >> 2;
  t |= t >> 1;
  return __popc(t & 0x01010101u);
}

// fast_count_mismatches(...) <= emax (merge_reads.cpp:195-236: only the comparison with the bound matters): a at any
// byte offset of a 4-aligned buffer, b 4-aligned, n bytes
__device__ __forceinline__ bool mg_prefilter(const uint8_t *abuf, int aoff, const uint8_t *b, int n, int emax) {
  const uint32_t *aw = (const uint32_t *)(abuf + (aoff & ~3));
  const uint32_t *bw = (const uint32_t *)b;
  const uint32_t sh = (uint32_t)(aoff & 3);
  const int nw = n >> 2, rem = n & 3;
  int mm = 0;
  uint32_t lo = aw[0];
  for (int w = 0; w < nw; w++) {
    const uint32_t hi = aw[w + 1];
    const uint32_t x = __builtin_amdgcn_alignbyte(hi, lo, sh) ^ bw[w];
    lo = hi;
    mm += mg_nonzero_bytes(x);
    if (mm > emax) return false;
  }
  if (rem) {
    const uint32_t x = (__builtin_amdgcn_alignbyte(aw[nw + 1], lo, sh) ^ bw[nw]) & ((1u << (8 * rem)) - 1u);
    mm += mg_nonzero_bytes(x);
  }
  return mm <= emax;
}

struct MgTrial {
  bool abort, good, weak;
};

// the exact loop of one trial (merge_reads.cpp:501-597's tests) at mate 1's position at = start_i + i.  Four bytes that
// equal their partners and hold no 'N' only add four matches, so they go by a word at a time; any other word goes
// byte by byte in source order.  ZERO: also write the N side's quality (:521, :529); the writes never change what this
// or another trial computes.
template <bool ZERO>
__device__ __forceinline__ MgTrial mg_exact(const MgBufs &b, int at, int overlap, int tmax, int emax) {
  int matches = 0, mism = 0, bothN = 0, ncount = 0, checked = 0;
  double perror = 0.0;
  bool abort = false, stop = false;
  const uint32_t *aw = (const uint32_t *)(b.s1 + (at & ~3));
  const uint32_t *bw = (const uint32_t *)b.rc;
  const uint32_t sh = (uint32_t)(at & 3);
  for (int j0 = 0; j0 < overlap && !stop; j0 += 4) {
    if (j0 + 4 <= overlap) {
      const uint32_t x = __builtin_amdgcn_alignbyte(aw[(j0 >> 2) + 1], aw[j0 >> 2], sh);
      const uint32_t y = x ^ 0x4E4E4E4Eu;  // a zero byte: an 'N'
      if (x == bw[j0 >> 2] && !((y - 0x01010101u) & ~y & 0x80808080u)) {
        matches += 4;
        checked += 4;
        continue;
      }
    }
    const int je = j0 + 4 < overlap ? j0 + 4 : overlap;
    for (int j = j0; j < je; j++) {
      checked++;
      const uint32_t ps = b.s1[at + j], rs = b.rc[j];
      if (ps == rs) {
        matches++;
        if (ps == 'N') {
          ncount += 2;
          if (bothN++) {
            abort = stop = true;
            break;
          }
        }
      } else {
        mism++;
        int qa = b.q1[at + j], qb = b.rq[j];
        if (ps == 'N') {
          mism++;
          ncount++;
          qa = 0;
          if (ZERO) b.q1[at + j] = 0;
          perror += b.pe[qb];
        } else if (rs == 'N') {
          ncount++;
          mism++;
          qb = 0;
          if (ZERO) b.rq[j] = 0;
          perror += b.pe[qa];
        }
        const int d = qa > qb ? qa - qb : qb - qa;
        perror += d <= 2 ? 0.5 : b.pe[d];
      }
      if (ncount > 3) {
        abort = stop = true;
        break;
      }
      if (mism > emax) {
        stop = true;
        break;
      }
    }
  }
  const double MAX_PERROR = 0.025;
  const int thres = overlap - tmax < MG_MIN_OVERLAP ? MG_MIN_OVERLAP : overlap - tmax;
  const double pe = perror / overlap;
  MgTrial r;
  r.abort = abort;
  r.good = matches >= thres && checked == overlap && mism <= tmax && pe <= MAX_PERROR;
  r.weak = !r.good && checked == overlap && mism <= emax && pe <= MAX_PERROR * 4 / 3;
  return r;
}

struct MgDecision {
  int best;  // -1: not merged
  int amb;   // num_ambiguous increments
};

__device__ __forceinline__ void mg_bounds(int overlap, int &tmax, int &emax) {
  tmax = MG_MAX_MISMATCHES + (MG_EXTRA_PER_1000 * overlap / 1000);
  emax = tmax * 4 / 3 + 1;
}

// the trial loop of one pair (wave-uniform result).  REPLAY: afterwards apply the executed trials' quality writes.
template <bool REPLAY>
__device__ __forceinline__ MgDecision mg_decide(const MgBufs &b, int len1, int len2, int lane) {
  const int len = len1 < len2 ? len1 : len2;
  const int start = len1 - len;
  const int ntr = len - MG_MIN_OVERLAP + MG_EXTRA_TEST_OVERLAP;
  int best = -1, found = -1, amb = 0, stop = ntr - 1;
  bool abort = false;
  for (int c0 = 0; c0 < ntr; c0 += 64) {
    const int i = c0 + lane;
    uint32_t ev = 0;
    if (i < ntr) {
      const int overlap = len - i;
      int tmax, emax;
      mg_bounds(overlap, tmax, emax);
      if (mg_prefilter(b.s1, start + i, b.rc, overlap, emax)) {
        const MgTrial t = mg_exact<false>(b, start + i, overlap, tmax, emax);
        ev = (t.abort ? 1u : 0u) | (t.good ? 2u : 0u) | (t.weak ? 4u : 0u);
      }
    }
    uint64_t m = __ballot(ev != 0);
    bool done = false;
    while (m) {  // the deciding trials of this chunk, in offset order (merge_reads.cpp:569-597)
      const int l = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const uint32_t e = __shfl(ev, l);
      const int ii = c0 + l;
      if (e & 1u) {
        abort = true;
        amb++;
      }
      if (e & 2u) {
        if (best < 0 && found < 0) {
          best = ii;
        } else {
          amb++;
          best = -1;
          done = true;
        }
      } else if (e & 4u) {
        found = ii;
        if (best >= 0) {
          amb++;
          best = -1;
          done = true;
        }
      }
      if (done || abort) {
        done = true;
        stop = ii;
        break;
      }
    }
    if (done) break;
  }
  if (REPLAY) {
    for (int c0 = 0; c0 <= stop; c0 += 64) {
      const int i = c0 + lane;
      if (i <= stop) {
        const int overlap = len - i;
        int tmax, emax;
        mg_bounds(overlap, tmax, emax);
        if (mg_prefilter(b.s1, start + i, b.rc, overlap, emax))
          (void)mg_exact<true>(b, start + i, overlap, tmax, emax);
      }
    }
    mg_wave_sync();
  }
  return MgDecision{abort ? -1 : best, amb};
}

// decision of pair p by one wave; lane 0 accumulates the statistics, returns its output bytes << 2 | reads
__device__ __forceinline__ uint32_t mg_decide_pair(const MergeArgs &a, uint64_t p, const MgBufs &b, int cap, int lane, uint64_t *st,
                                                   bool is_long) {
  uint64_t o1, o2;
  int len1 = 0, len2 = 0;
  if (!mg_pair(a, p, o1, o2, len1, len2)) {
    if (lane == 0) {
      atomicOr(&a.ctl[MG_CTL_ERR], (uint32_t)MG_ERR_ARG);
      a.pair_dec[p] = 0;
      a.pair_out[p] = 0;
    }
    return 0;
  }
  if (!is_long && (len1 > cap || len2 > cap)) {
    if (lane == 0) {
      const uint32_t at = atomicAdd(&a.ctl[MG_CTL_NLONG], 1u);
      a.long_list[at] = (uint32_t)p;
      atomicMax(&a.ctl[MG_CTL_LONGMAX], (uint32_t)(len1 > len2 ? len1 : len2));
      a.pair_dec[p] = MG_DEC_LONG;
      a.pair_out[p] = 0;
    }
    return 0;
  }
  uint32_t dec, out;
  if (len1 < a.min_len && len2 < a.min_len) {  // merge_reads.cpp:473 (the bytes are still checked)
    bool anyN;
    const uint32_t err = is_long ? mg_load<false>(a, b, o1, o2, len1, len2, lane, anyN) : mg_load<true>(a, b, o1, o2, len1, len2, lane, anyN);
    if (err && lane == 0) atomicOr(&a.ctl[MG_CTL_ERR], err);
    dec = 0;
    out = 0;
    if (lane == 0) st[MGS_DROPPED]++;
  } else {
    bool anyN;
    const uint32_t err = is_long ? mg_load<false>(a, b, o1, o2, len1, len2, lane, anyN) : mg_load<true>(a, b, o1, o2, len1, len2, lane, anyN);
    if (err) {
      if (lane == 0) atomicOr(&a.ctl[MG_CTL_ERR], err);
      dec = 0;
      out = 0;
    } else {
      const MgDecision d = mg_decide<false>(b, len1, len2, lane);
      dec = (uint32_t)(d.best + 2) | (anyN ? MG_DEC_REPLAY : 0u);
      if (d.best >= 0) {
        const int len = len1 < len2 ? len1 : len2;
        const int mlen = (len1 - len) + d.best + len2;
        out = ((uint32_t)mlen << 2) | 1u;
        if (lane == 0) {
          st[MGS_MERGED]++;
          st[MGS_OVERLAP] += (uint64_t)(len - d.best);
          st[MGS_MERGED_LEN] += (uint64_t)mlen;
        }
      } else {
        out = ((uint32_t)(len1 + len2) << 2) | 2u;
      }
      if (lane == 0) st[MGS_AMBIG] += (uint64_t)d.amb;
    }
  }
  mg_wave_sync();  // the next pair reuses the buffers
  if (lane == 0) {
    a.pair_dec[p] = dec | (is_long ? MG_DEC_LONG : 0u);
    a.pair_out[p] = out;
  }
  return out;
}

__device__ __forceinline__ void mg_flush_stats(const MergeArgs &a, const uint64_t *st) {
  uint64_t *s = a.stats + (size_t)(blockIdx.x % MG_SLOTS) * MGS_N;
  for (int f = 0; f < MGS_N; f++)
    if (st[f]) atomicAdd((unsigned long long *)&s[f], (unsigned long long)st[f]);
}

__global__ void __launch_bounds__(64 * MG_WAVES) kc_merge_decide_kernel(MergeArgs a) {
  __shared__ double pe[81];
  mg_load_table(pe);
  __shared__ __attribute__((aligned(16))) uint8_t lds[MG_WAVES][4 * (MG_MAXL + MG_PAD)];
  __shared__ uint64_t wsum[MG_WAVES][2 + MGS_N];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const MgBufs b = mg_bufs(lds[wv], MG_MAXL, pe);
  uint64_t st[MGS_N] = {0, 0, 0, 0, 0};
  uint64_t bytes = 0, reads = 0;
  const uint64_t p0 = (uint64_t)blockIdx.x * MG_TILE;
  for (int k = wv; k < MG_TILE; k += MG_WAVES) {
    const uint64_t p = p0 + k;
    if (p >= a.npairs) break;
    const uint32_t out = mg_decide_pair(a, p, b, MG_MAXL, lane, st, false);
    bytes += out >> 2;
    reads += out & 3u;
  }
  if (lane == 0) {
    wsum[wv][0] = bytes;
    wsum[wv][1] = reads;
    for (int f = 0; f < MGS_N; f++) wsum[wv][2 + f] = st[f];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s[2 + MGS_N];
    for (int f = 0; f < 2 + MGS_N; f++) {
      s[f] = 0;
      for (int w = 0; w < MG_WAVES; w++) s[f] += wsum[w][f];
    }
    a.tile_bytes[blockIdx.x] = s[0];
    a.tile_reads[blockIdx.x] = s[1];
    mg_flush_stats(a, s + 2);
  }
}

// the listed long pairs: one wave per workgroup, the mates in dynamic LDS of 4 * (cap + MG_PAD) bytes
__global__ void __launch_bounds__(64) kc_merge_decide_long_kernel(MergeArgs a, int cap) {
  __shared__ double pe[81];
  mg_load_table(pe);
  extern __shared__ __attribute__((aligned(16))) uint8_t dlds[];
  const int lane = threadIdx.x;
  const uint64_t p = a.long_list[blockIdx.x];
  uint64_t st[MGS_N] = {0, 0, 0, 0, 0};
  const uint32_t out = mg_decide_pair(a, p, mg_bufs(dlds, cap, pe), cap, lane, st, true);
  if (lane == 0) {
    atomicAdd((unsigned long long *)&a.tile_bytes[p / MG_TILE], (unsigned long long)(out >> 2));
    atomicAdd((unsigned long long *)&a.tile_reads[p / MG_TILE], (unsigned long long)(out & 3u));
    mg_flush_stats(a, st);
  }
}

// output of pair p from the wave's LDS copy; obase / rbase: its first output byte and read
__device__ __forceinline__ void mg_write_pair(const MergeArgs &a, uint64_t p, uint32_t dec, const MgBufs &b, int lane, uint64_t obase,
                                              uint64_t rbase, bool is_long) {
  uint64_t o1, o2;
  int len1, len2;
  (void)mg_pair(a, p, o1, o2, len1, len2);
  bool anyN;
  if (is_long)
    (void)mg_load<false>(a, b, o1, o2, len1, len2, lane, anyN);
  else
    (void)mg_load<true>(a, b, o1, o2, len1, len2, lane, anyN);
  int best = (int)(dec & 0xFFFFu) - 2;
  if (dec & MG_DEC_REPLAY) best = mg_decide<true>(b, len1, len2, lane).best;
  if (best >= 0) {
    const int len = len1 < len2 ? len1 : len2;
    const int at = (len1 - len) + best;  // first position of the overlap in mate 1
    const int mlen = at + len2;
    for (int t = lane; t < mlen; t += 64) {
      uint32_t c, q;
      if (t < at) {
        c = b.s1[t];
        q = b.q1[t];
      } else if (t < len1) {  // merge_reads.cpp:604-624
        const int j = t - at;
        const uint32_t c1 = b.s1[t], c2 = b.rc[j], q1 = b.q1[t], q2 = b.rq[j];
        if (c1 == c2) {
          c = c1;
          q = q1 + q2 > (uint32_t)MG_MAX_MATCH_QUAL ? (uint32_t)MG_MAX_MATCH_QUAL : q1 + q2;
        } else {
          c = q1 < q2 ? c2 : c1;
          q = q1 < q2 ? q2 - q1 : q1 - q2;
          q = q > 2u ? q : 2u;
        }
      } else {
        c = b.rc[t - at];
        q = b.rq[t - at];
      }
      a.out[obase + t] = (uint8_t)(mg_code(c) | ((q > 31u ? 31u : q) << 3));
    }
    if (lane == 0) a.out_offsets[rbase + 1] = obase + mlen;
  } else {
    for (int t = lane; t < len1; t += 64) {
      const uint32_t q = b.q1[t];
      a.out[obase + t] = (uint8_t)(mg_code(b.s1[t]) | ((q > 31u ? 31u : q) << 3));
    }
    for (int t = lane; t < len2; t += 64) {  // mate 2 as it came, with its own qualities (not rev_quals2)
      const uint32_t q = (uint32_t)((int)a.quals[o2 + t] - a.qoff);
      a.out[obase + len1 + t] = (uint8_t)(mg_code(a.bases[o2 + t]) | ((q > 31u ? 31u : q) << 3));
    }
    if (lane == 0) {
      a.out_offsets[rbase + 1] = obase + len1;
      a.out_offsets[rbase + 2] = obase + len1 + len2;
    }
  }
  mg_wave_sync();
}

__global__ void __launch_bounds__(64 * MG_WAVES) kc_merge_write_kernel(MergeArgs a) {
  __shared__ double pe[81];
  mg_load_table(pe);
  __shared__ __attribute__((aligned(16))) uint8_t lds[MG_WAVES][4 * (MG_MAXL + MG_PAD)];
  __shared__ uint64_t ob[MG_TILE], orr[MG_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * MG_TILE;
  if (wv == 0) {  // in-tile exclusive offsets
    const uint64_t p = p0 + lane;
    const uint32_t o = p < a.npairs ? a.pair_out[p] : 0u;
    uint64_t ib = o >> 2, ir = o & 3u;
    for (int s = 1; s < 64; s <<= 1) {
      const uint64_t tb = __shfl_up(ib, s), tr = __shfl_up(ir, s);
      if (lane >= s) {
        ib += tb;
        ir += tr;
      }
    }
    ob[lane] = a.tile_bytes[blockIdx.x] + ib - (o >> 2);
    orr[lane] = a.tile_reads[blockIdx.x] + ir - (o & 3u);
  }
  __syncthreads();
  const MgBufs b = mg_bufs(lds[wv], MG_MAXL, pe);
  for (int k = wv; k < MG_TILE; k += MG_WAVES) {
    const uint64_t p = p0 + k;
    if (p >= a.npairs) break;
    const uint32_t dec = a.pair_dec[p];
    if ((dec & 0xFFFFu) == 0 || (dec & MG_DEC_LONG)) continue;  // dropped, or written by the long kernel
    mg_write_pair(a, p, dec, b, lane, ob[k], orr[k], false);
  }
}

__global__ void __launch_bounds__(64) kc_merge_write_long_kernel(MergeArgs a, int cap) {
  __shared__ double pe[81];
  mg_load_table(pe);
  extern __shared__ __attribute__((aligned(16))) uint8_t dlds[];
  const int lane = threadIdx.x;
  const uint64_t p = a.long_list[blockIdx.x];
  const uint32_t dec = a.pair_dec[p];
  const uint64_t tile = p / MG_TILE, p0 = tile * MG_TILE;
  const uint64_t q = p0 + lane;
  const uint32_t o = q < p ? a.pair_out[q] : 0u;  // the pairs in front of p in its tile
  uint64_t sb = o >> 2, sr = o & 3u;
  for (int s = 1; s < 64; s <<= 1) {
    sb += __shfl_xor(sb, s);
    sr += __shfl_xor(sr, s);
  }
  if ((dec & 0xFFFFu) == 0) return;
  mg_write_pair(a, p, dec, mg_bufs(dlds, cap, pe), lane, a.tile_bytes[tile] + sb, a.tile_reads[tile] + sr, true);
}

}  // namespace kc
