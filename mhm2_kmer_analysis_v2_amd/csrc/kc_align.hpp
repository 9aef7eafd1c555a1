// kc_align.hpp -- reads back onto contigs (the role of find_alignments, src/contigging.cpp:150-163, commented out in the
// proxy like the traversal before it).  The reference holds no alignment code, so the rules are this project's own
// (pinned statement by statement by tests/align_model.py): an exact seed index over a '_'-joined
// block of contigs -- a canonical k-mer is a seed iff exactly one window of the whole block has it and it is not its own
// reverse complement -- and, per read, every (contig, orient, diagonal) some seed of the read votes for, checked
// without gaps over the whole overlap.
//
// Index: an open-addressing table of 64-bit slots, at most half full.  A slot identifies its k-mer by the text it
// points at, not by a stored key:
//   bits  0..31  block position of the window + 1 (0 = empty)
//   bit   32     strand: the contig window is its own canonical form
//   bit   33     repeated: a second window (or the window's own reverse complement) has the key -- only ever set
//   bits 34..63  the upper 30 bits of the key's hash, so that a probe reads contig text only where they agree
// Which position a repeated slot keeps depends on arrival order and is never read; whether a slot is repeated does not.
#pragma once
#include "kc_common.hpp"
#include "kc_kit.hpp"

namespace kc {

constexpr int ALIGN_MAX_READ_LEN = 1024;  // KC_ALIGN_MAX_READ_LEN
constexpr int ALIGN_TPB = 256;
constexpr int ALIGN_WAVES = ALIGN_TPB / 64;  // reads of a workgroup, a wave each
constexpr int ALIGN_CODE_WORDS = 40;         // 32 words of 2-bit codes + the words a window at the very end reaches into
constexpr int ALIGN_MASK_WORDS = 20;         // 16 words of no-base bits + the same
constexpr uint64_t AI_STRAND = 1ull << 32, AI_REPEATED = 1ull << 33;
constexpr int AI_TAG_SHIFT = 34;
constexpr int64_t ALIGN_D_BIAS = ALIGN_MAX_READ_LEN;  // d > -1024, so d + bias is a positive 32-bit number
constexpr uint64_t ALIGN_NO_CAND = ~0ull;

// status words of the index build / counters of an align call
enum { AIS_BAD_BASE = 0, AIS_BAD_OFFSETS, AIS_SEPARATORS, AIS_WINDOWS, AIS_SEEDS, AIS_REPEATED, AIS_COUNT };
enum { ALS_BAD_READ = 0, ALS_MAX_LEN, ALS_READS_ALIGNED, ALS_WINDOWS, ALS_SEED_HITS, ALS_REPEATED_HITS, ALS_ALIGNMENTS, ALS_PERFECT,
       ALS_TOTAL, ALS_COUNT };

struct AlignIndex {
  const uint8_t *seqs;    // the block
  const uint32_t *offs;   // n_ctgs + 1 starts
  const uint64_t *slots;
  uint64_t mask;          // slots - 1
  uint32_t n_ctgs;
};

// A C G T in upper case only: a contig's N is no base here, and '_' ends every window
__device__ __forceinline__ bool ai_is_acgt_upper(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// the k characters at s as a forward k-mer; false if one of them is not ACGT
template <int NL>
__device__ __forceinline__ bool ai_pack(const uint8_t *s, int k, uint64_t (&f)[NL]) {
#pragma unroll
  for (int j = 0; j < NL; j++) f[j] = 0;
  bool ok = true;
  for (int i = 0; i < k; i++) {
    const uint32_t ch = s[i];
    ok &= ai_is_acgt_upper(ch);
    const uint64_t code = (uint64_t)kc_base_code(ch) << (62 - 2 * (i & 31));
#pragma unroll
    for (int j = 0; j < NL; j++)
      if (j == (i >> 5)) f[j] |= code;
  }
  return ok;
}

// kc_revcomp for NL = kc_record_longs(k) words, without its per-word selects (in the reads kernel's window loop each of
// them is a lane mask held in scalar registers): reverse and complement all NL words, then shift the 64 NL bits left by
// the 64 NL - 2k that are no bases -- fewer than 128, so a bit shift and at most one word.  The complemented padding
// leaves at the front, zeros come in at the back.
template <int NL>
KC_HD void ai_revcomp(const uint64_t (&w)[NL], int k, uint64_t (&out)[NL]) {
  uint64_t t[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) t[i] = kc_rc_word(w[NL - 1 - i]);
  const int total = 64 * NL - 2 * k, bs = total & 63;
  if (bs) {
#pragma unroll
    for (int j = 0; j < NL; j++) t[j] = (t[j] << bs) | ((j + 1 < NL ? t[j + 1] : 0ULL) >> (64 - bs));
  }
  const bool word = total >= 64;
#pragma unroll
  for (int j = 0; j < NL; j++) out[j] = word ? (j + 1 < NL ? t[j + 1] : 0ULL) : t[j];
}

template <int NL>
__device__ __forceinline__ bool ai_equal(const uint64_t (&a)[NL], const uint64_t (&b)[NL]) {
  bool same = true;
#pragma unroll
  for (int j = 0; j < NL; j++) same &= a[j] == b[j];
  return same;
}

// Alphabet, separators and offsets of a block, position by position and contig by contig; offs32 receives the offsets
// in 32 bits.  Every offset is compared with nbytes before the byte in front of it is read.
__global__ void kc_align_check_kernel(const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, uint32_t *offs32,
                                      uint64_t *status) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool sep = false;
  if (t < nbytes) {
    const uint32_t c = seqs[t];
    sep = c == '_';
    if (!sep && !ai_is_acgt_upper(c) && c != 'N') status[AIS_BAD_BASE] = 1;
  }
  const uint32_t nsep = wave_count(sep);
  if ((threadIdx.x & 63) == 0 && nsep) atomicAdd((unsigned long long *)&status[AIS_SEPARATORS], (unsigned long long)nsep);
  if (t <= n_ctgs) {
    const uint64_t o = offsets[t];
    bool ok = o <= nbytes;
    if (t == 0) ok &= o == 0;
    if (t == n_ctgs) {
      ok &= o == nbytes;
    } else {
      const uint64_t nxt = offsets[t + 1];
      ok &= nxt > o && nxt <= nbytes;
      if (ok) ok = seqs[nxt - 1] == '_';
    }
    if (!ok) status[AIS_BAD_OFFSETS] = 1;
    offs32[t] = (uint32_t)o;
  }
}

// One thread per block position: its window, if it is one, goes into the table.
template <int NL>
__global__ void kc_align_index_kernel(const uint8_t *seqs, uint32_t nbytes, int k, uint64_t *slots, uint64_t mask, uint64_t *status) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t f[NL], r[NL];
  bool window = p + (uint64_t)k <= nbytes;
  if (window) window = ai_pack<NL>(seqs + p, k, f);
  const uint32_t nw = wave_count(window);
  if ((threadIdx.x & 63) == 0 && nw) atomicAdd((unsigned long long *)&status[AIS_WINDOWS], (unsigned long long)nw);
  if (!window) return;
  kc_revcomp<NL>(f, k, r);
  const bool swap = kc_less<NL>(r, f);  // strict, as in S4
  const bool palindrome = ai_equal<NL>(f, r);
  if (swap) {
#pragma unroll
    for (int j = 0; j < NL; j++) f[j] = r[j];
  }
  const uint64_t h = kc_hash<NL>(f);
  const uint64_t entry = ((h >> AI_TAG_SHIFT) << AI_TAG_SHIFT) | (palindrome ? AI_REPEATED : 0) | (swap ? 0 : AI_STRAND) | (p + 1);
  for (uint64_t s = h & mask;; s = (s + 1) & mask) {  // at most half the slots are ever taken: an empty one ends the chain
    const uint64_t old = atomicCAS((unsigned long long *)&slots[s], 0ULL, (unsigned long long)entry);
    if (old == 0) return;
    if ((old >> AI_TAG_SHIFT) != (h >> AI_TAG_SHIFT)) continue;
    uint64_t g[NL], gr[NL];
    (void)ai_pack<NL>(seqs + ((uint32_t)old - 1u), k, g);  // a slot's position is a window: all bases
    if (!(old & AI_STRAND)) {
      kc_revcomp<NL>(g, k, gr);
#pragma unroll
      for (int j = 0; j < NL; j++) g[j] = gr[j];
    }
    if (ai_equal<NL>(g, f)) {
      if (!(old & AI_REPEATED)) atomicOr((unsigned long long *)&slots[s], (unsigned long long)AI_REPEATED);
      return;
    }
  }
}

__global__ void kc_align_sweep_kernel(const uint64_t *slots, uint64_t n, uint64_t *status) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t e = s < n ? slots[s] : 0;
  const uint32_t seeds = wave_count(e != 0 && !(e & AI_REPEATED)), rep = wave_count(e != 0 && (e & AI_REPEATED));
  if ((threadIdx.x & 63) == 0) {
    if (seeds) atomicAdd((unsigned long long *)&status[AIS_SEEDS], (unsigned long long)seeds);
    if (rep) atomicAdd((unsigned long long *)&status[AIS_REPEATED], (unsigned long long)rep);
  }
}

// The longest read, and the first one over the limit (or with offsets that go backwards): st[ALS_BAD_READ] starts at ~0.
__global__ void kc_align_lengths_kernel(const uint64_t *offsets, uint64_t nreads, uint64_t *st) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t len = 0;
  bool bad = false;
  if (r < nreads) {
    const uint64_t a = offsets[r], b = offsets[r + 1];
    bad = b < a || b - a > (uint64_t)ALIGN_MAX_READ_LEN;
    len = bad ? 0 : b - a;
  }
  if (bad) atomicMin((unsigned long long *)&st[ALS_BAD_READ], (unsigned long long)r);
  len = wave_max(len);
  if ((threadIdx.x & 63) == 0 && len) atomicMax((unsigned long long *)&st[ALS_MAX_LEN], (unsigned long long)len);
}

// A wave per read.  WPL: windows a lane holds (the host picks the smallest class the longest read of the call fits).
// alns == nullptr: the count pass -- first[read] = the read's emitted candidates, and the call's statistics.
// Otherwise the write pass, after the scan of first: the same work again, records written from first[read] on.
template <int NL, int WPL>
__global__ void __launch_bounds__(ALIGN_TPB) kc_align_reads_kernel(AlignIndex ix, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads,
                                                                   int k, uint32_t seed_space, uint32_t max_mismatches, uint64_t *first,
                                                                   uint4 *alns, uint64_t *st) {
  __shared__ __attribute__((aligned(8))) uint32_t codes32[ALIGN_WAVES][2 * ALIGN_CODE_WORDS];
  __shared__ __attribute__((aligned(8))) uint16_t mask16[ALIGN_WAVES][4 * ALIGN_MASK_WORDS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t read = (uint64_t)blockIdx.x * ALIGN_WAVES + wv;
  const bool live = read < nreads;
  const uint64_t r0 = live ? offsets[read] : 0;
  const uint32_t L = live ? (uint32_t)(offsets[read + 1] - r0) : 0u;  // <= ALIGN_MAX_READ_LEN (kc_align_lengths_kernel)
  // ---- the read, once: 2-bit codes in the k-mer's own layout (base j in bits 63-2(j%32)-1.. of word j/32) and one
  // no-base bit per position (bit j%64 of word j/64); everything behind the read is "no base"
  {
    uint32_t cw = 0, mw = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t idx = 16u * lane + i;
      const uint32_t c = idx < L ? bases[r0 + idx] : 0u;
      if (kc_is_acgt(c))
        cw |= kc_base_code(c) << (30 - 2 * i);
      else
        mw |= 1u << i;
    }
    codes32[wv][lane ^ 1] = cw;  // the upper half of a 64-bit word holds its first 16 bases
    mask16[wv][lane] = (uint16_t)mw;
    if (lane < 2 * ALIGN_CODE_WORDS - 64) codes32[wv][64 + lane] = 0;
    if (lane < 4 * ALIGN_MASK_WORDS - 64) mask16[wv][64 + lane] = 0xFFFFu;
  }
  __syncthreads();
  const uint64_t *codes = (const uint64_t *)codes32[wv];
  const uint64_t *nobase = (const uint64_t *)mask16[wv];

  // ---- seeds: lane's windows p = s (lane + 64 i), cut out of the staged words with shifts
  uint64_t cand[WPL];
#pragma unroll
  for (int j = 0; j < WPL; j++) cand[j] = ALIGN_NO_CAND;
  uint32_t n_look = 0, n_hit = 0, n_rep = 0;
  const uint32_t nstarts = L >= (uint32_t)k ? (L - (uint32_t)k) / seed_space + 1u : 0u;
#pragma unroll 1
  for (int i = 0; i < WPL; i++) {
    if ((uint32_t)(64 * i) >= nstarts) break;  // the same for the whole wave
    const uint32_t idx = (uint32_t)lane + 64u * i;
    const uint32_t p = idx < nstarts ? idx * seed_space : 0u;  // idx < nstarts: p <= L - k
    bool valid = idx < nstarts;
    {  // no "no base" among the k positions from p on
      const uint32_t w = p >> 6, sh = p & 63u;
      uint64_t any = 0;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int nb = k - 64 * j;
        if (nb > 0) {
          const uint64_t m = sh ? (nobase[w + j] >> sh) | (nobase[w + j + 1] << (64u - sh)) : nobase[w + j];
          any |= nb >= 64 ? m : m & ((1ull << nb) - 1ull);
        }
      }
      valid &= any == 0;
    }
    uint64_t c = ALIGN_NO_CAND;
    bool hit = false, rep = false;
    if (valid) {
      uint64_t f[NL], r[NL];
      const uint32_t w = p >> 5, sh = 2u * (p & 31u);
#pragma unroll
      for (int j = 0; j < NL; j++) {
        const uint64_t hi = codes[w + j], lo = codes[w + j + 1];
        f[j] = (sh ? (hi << sh) | (lo >> (64u - sh)) : hi) & kc_word_mask(k, j);
      }
      ai_revcomp<NL>(f, k, r);
      const bool rswap = kc_less<NL>(r, f);
      const uint64_t h = rswap ? kc_hash<NL>(r) : kc_hash<NL>(f);
      for (uint64_t s = h & ix.mask;; s = (s + 1) & ix.mask) {
        const uint64_t e = ix.slots[s];
        if (e == 0) break;
        if ((e >> AI_TAG_SHIFT) != (h >> AI_TAG_SHIFT)) continue;
        const uint32_t pos = (uint32_t)e - 1u;
        // the contig text y is the read's window as it stands (orient 0) or reverse-complemented (orient 1): which one a
        // slot with this key holds follows from the two strand bits
        const bool orient = ((e & AI_STRAND) != 0) == rswap;
        uint64_t y[NL];
        (void)ai_pack<NL>(ix.seqs + pos, k, y);
        if (!(orient ? ai_equal<NL>(y, r) : ai_equal<NL>(y, f))) continue;
        if (e & AI_REPEATED) {
          rep = true;
          break;
        }
        hit = true;
        const uint32_t lo = find_le(ix.offs, 0u, ix.n_ctgs - 1u, pos);  // the contig: the last one that starts at or before pos
        const int64_t j = (int64_t)pos - (int64_t)ix.offs[lo];
        const int64_t d = j - (orient ? (int64_t)(L - (uint32_t)k - p) : (int64_t)p);
        c = ((uint64_t)lo << 33) | ((uint64_t)(orient ? 1u : 0u) << 32) | (uint64_t)(uint32_t)(d + ALIGN_D_BIAS);
        break;
      }
    }
    n_look += wave_count(valid);
    n_hit += wave_count(hit);
    n_rep += wave_count(rep);
#pragma unroll
    for (int j = 0; j < WPL; j++)
      if (j == i) cand[j] = c;
  }

  // ---- distinct candidates in ascending order: the wave's smallest key, its votes, its mismatches, emit, retire
  const uint64_t out0 = (alns && live) ? first[read] : 0;
  uint32_t n_emit = 0, n_perfect = 0;
  for (;;) {
    uint64_t m = cand[0];
#pragma unroll
    for (int j = 1; j < WPL; j++) m = cand[j] < m ? cand[j] : m;
    m = wave_min(m);
    if (m == ALIGN_NO_CAND) break;
    uint32_t votes = 0;
#pragma unroll
    for (int j = 0; j < WPL; j++) {
      const bool mine = cand[j] == m;
      votes += wave_count(mine);
      cand[j] = mine ? ALIGN_NO_CAND : cand[j];
    }
    const uint32_t u = (uint32_t)(m >> 33);
    const bool orient = (m >> 32) & 1u;
    const int64_t d = (int64_t)(uint32_t)m - ALIGN_D_BIAS;
    const uint32_t c0 = ix.offs[u];
    const int64_t len = (int64_t)(ix.offs[u + 1] - 1u - c0);
    const int64_t cstart = d > 0 ? d : 0, cstop = d + (int64_t)L < len ? d + (int64_t)L : len;
    const uint32_t rstart = (uint32_t)(cstart - d), rstop = (uint32_t)(cstop - d);
    const int64_t cbase = (int64_t)c0 + d;  // block position that pairs with R'[0]; only [rstart, rstop) is read
    uint32_t mism = 0;
    for (uint32_t b = rstart; b < rstop; b += 64u) {
      const uint32_t i = b + (uint32_t)lane;
      bool bad = false;
      if (i < rstop) {
        const uint32_t ri = orient ? L - 1u - i : i;
        uint32_t code = (uint32_t)(codes[ri >> 5] >> (62u - 2u * (ri & 31u))) & 3u;
        if (orient) code = 3u - code;
        const bool nb = (nobase[ri >> 6] >> (ri & 63u)) & 1u;
        const uint32_t cb = ix.seqs[cbase + (int64_t)i];
        bad = nb || cb == 'N' || kc_base_code(cb) != code;
      }
      mism += wave_count(bad);
    }
    if (mism <= max_mismatches) {
      if (alns && lane == 0) {
        uint4 a, z;
        a.x = (uint32_t)read;
        a.y = u;
        a.z = (uint32_t)cstart;
        a.w = (uint32_t)cstop;
        z.x = rstart | (rstop << 16);
        z.y = mism | (votes << 16);
        z.z = orient ? 1u : 0u;
        z.w = 0;
        alns[2 * (out0 + n_emit)] = a;
        alns[2 * (out0 + n_emit) + 1] = z;
      }
      n_emit++;
      n_perfect += (mism == 0 && rstart == 0 && rstop == L) ? 1u : 0u;
    }
  }
  if (!alns && live && lane == 0) {
    first[read] = n_emit;
    auto add = [&](int which, uint32_t v) {
      if (v) atomicAdd((unsigned long long *)&st[which], (unsigned long long)v);
    };
    add(ALS_READS_ALIGNED, n_emit ? 1u : 0u);
    add(ALS_WINDOWS, n_look);
    add(ALS_SEED_HITS, n_hit);
    add(ALS_REPEATED_HITS, n_rep);
    add(ALS_ALIGNMENTS, n_emit);
    add(ALS_PERFECT, n_perfect);
  }
}

}  // namespace kc
