// kc_lassm.hpp -- contig ends extended by local assembly (kc_local_assm): the role of localassm(LASSM_MAX_KMER_LEN, kmer_len,
// packed_reads_list, ins_avg, ins_stddev, qual_offset, ctgs, alns), src/contigging.cpp:167-172, commented out in the proxy
// like the steps before it.  The reference holds no code for it (no localassm in src/), so the rules are this project's
// own definition (pinned statement by statement by tests/lassm_model.py); no parity with MetaHipMer
// is claimed.  include/kcount_mi355.h states the rules in full.
//
// Ends: end 2u is the left end of contig u, end 2u + 1 its right end.  Every walk runs rightwards: a left end is the right
// end of the contig's reverse complement, so the candidates of a left end are stored reverse-complemented.
//
// Kernels:
//  kc_lassm_pair_check_kernel  a thread per pair: the validity of its two record indices, the lowest bad pair by a 64-bit
//                              atomicMin.  Stores nothing else.
//  kc_lassm_cands_kernel<W>    a thread per read, run twice.  W = false counts, per end, the candidates and their bases;
//                              W = true reserves an entry and a piece of the end's text through two atomic cursors and
//                              writes the 16-byte entry {read << 1 | revcomp, end, text start, length}.  The order of an
//                              end's candidates is left free: every result is a sum of integers over them.
//  kc_lassm_plan_kernel        a thread per end: NO_CANDS / TOO_MANY, and for the others the entries, the text bytes
//                              (bases + one separator a candidate) and the table slots (the power of two at or above
//                              twice the bases: the windows are fewer than the bases, so a table is at most half full);
//                              kc_scan_kernel<2> and <1> (kc_scan.hpp) turn the three into offsets.
//  kc_lassm_text_kernel        a thread per entry writes the candidate in walk orientation, once: a byte code | class << 3
//                              a base (code 4: no base; the separator behind a candidate is one), a byte with the run of
//                              bases that starts there (capped at 255 > KC_LASSM_MAX_MER_LEN + 1) and the 64-bit prefix of
//                              a polynomial hash -- so the walk kernel knows a window's validity from one byte and its
//                              hash from two words, whatever the mer length, and holds no orientation logic.
//  kc_lassm_walk_kernel        a wave per end (workgroups of one wave), every iteration of the end:
//      clear   the wave zeroes its own table (40-byte slots: text position + 1, visited stamp, hi[4], lo[4]).
//      build   lanes take text positions; a window is a mer iff the run of bases there is longer than m and the byte
//              behind it has a class.  The slot's key is a text position claimed by one atomicCAS; a lane that finds the
//              slot taken compares text.  Nothing waits on another lane: a CAS result is final at once.  Counters are
//              32-bit atomicAdds.
//      steps   the current mer is the last m codes of a 128-byte ring in LDS (the tail, then the extension); its hash
//              rolls.  A slot's ten words are loaded at once; the lanes compare the mer with the text the slot points
//              at, two bytes a lane, and vote.  Lane 0 sets the visited stamp and its own load of it is the one that
//              counts; every decision is computed from values all lanes hold alike.
//      Device-scope fences stand between clear, build and steps (the atomics work in L2; the fence makes the wave's plain
//      stores visible there and drops its L1 lines).  Every loop's trip count is bounded by the input: the slots, the
//      text, max_walk_len, and the iterations by (max_mer_len - min_mer_len) / shift + 1, for the mer length moves one
//      way only.  There are no spins.
//  kc_lassm_lens_kernel        a thread per contig: the new length and the statistics; kc_scan_kernel<1> gives the offsets.
//  kc_lassm_ends_kernel        a thread per end: the 16-byte record, one store.
//  kc_lassm_write_kernel       a thread per 16 bytes of the new block: left extension reversed and complemented, the contig
//                              as it is, the right extension, the separator; one 16-byte store where the array's
//                              alignment and its end allow.
#pragma once
#include "kc_depth.hpp"

namespace kc {

constexpr uint32_t LASSM_MAX_MER = 128;         // KC_LASSM_MAX_MER_LEN
constexpr uint32_t LASSM_MAX_WALK = 4096;       // KC_LASSM_MAX_WALK
constexpr uint32_t LASSM_MAX_CANDS = 1u << 20;  // KC_LASSM_MAX_CANDS
constexpr uint32_t LASSM_NO_CANDS = 0, LASSM_TOO_MANY = 1, LASSM_DEAD_END = 2, LASSM_FORK = 3, LASSM_LOOP = 4, LASSM_MAX_LEN = 5;
constexpr int LASSM_STATUSES = 6;
constexpr uint32_t LASSM_CLS_NONE = 0, LASSM_CLS_LO = 1, LASSM_CLS_HI = 2;
constexpr uint32_t LASSM_SLOT_WORDS = 10;  // key, stamp, hi[4], lo[4]
constexpr uint64_t LASSM_HASH_BASE = 0xD6E8FEB86659FD93ull;
constexpr uint32_t LASSM_NO_ALN = 0xFFFFFFFFu;

enum { LS_BAD_PAIR = 0, LS_OVERHANG, LS_MATE, LS_CAND_BASES, LS_ENT_TOTAL, LS_TEXT_TOTAL, LS_SLOT_TOTAL, LS_STATUS,
       LS_ITERS = LS_STATUS + LASSM_STATUSES, LS_EXT_BASES, LS_EXTENDED, LS_OUT_TOTAL, LS_COUNT };

struct LassmArgs {
  const uint8_t *seqs;   // the index's block
  const uint32_t *offs;  // its n_ctgs + 1 starts
  uint32_t n_ctgs, n_ends;
  const uint8_t *bases, *quals;  // quals may be null
  const uint64_t *offsets;
  uint64_t nreads;
  const uint4 *alns;  // kc_gap_aln
  uint64_t n_alns;
  const uint4 *pairs;  // kc_pair_rec
  const uint4 *ctgs;   // kc_ctg_depth or null
  uint32_t k, min_mer, max_mer, shift, max_walk, max_insert, min_viable, permille, max_cands;
  int min_q, hi_q;  // as quality bytes: the offset is added
  uint64_t *st;
  uint64_t *e_cands, *e_bases;          // [n_ends] counted
  uint64_t *e_ent, *e_text, *e_slots;   // [n_ends] planned, then scanned
  uint32_t *e_ecur, *e_tcur;            // [n_ends] cursors of the second candidate pass
  uint4 *e_res;                         // [n_ends] {status, ext_len, iters, mer_len}
  uint4 *entries;
  uint8_t *tcode, *tnb;
  uint64_t *tph;
  uint32_t *table;
  uint8_t *ext;      // [n_ends * max_walk] the extensions as A C G T, in walk orientation
  uint64_t *newoff;  // [n_ctgs + 1]
};

__device__ __forceinline__ uint32_t lassm_class(const LassmArgs &a, uint64_t at) {
  if (!a.quals) return LASSM_CLS_HI;
  const int q = (int)a.quals[at];
  return q >= a.hi_q ? LASSM_CLS_HI : q >= a.min_q ? LASSM_CLS_LO : LASSM_CLS_NONE;
}

__device__ __forceinline__ uint32_t lassm_slot(uint64_t h) { return (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 33); }

// the slots of an end with b >= 1 candidate bases (b <= 2^30): the power of two at or above 2 b
__device__ __forceinline__ uint64_t lassm_slots(uint64_t b) { return 1ull << (64 - __clzll((long long)(2 * b - 1))); }

__device__ __forceinline__ uint32_t lassm_ld(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void kc_lassm_pair_check_kernel(LassmArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nreads / 2) return;
  const uint4 pr = a.pairs[p];
  bool ok = true;
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const uint32_t i = side ? pr.y : pr.x;
    if (i == LASSM_NO_ALN) continue;
    if ((uint64_t)i >= a.n_alns) {
      ok = false;
      continue;
    }
    const DepthRec r = depth_load(a.alns, i);
    ok = ok && (uint64_t)r.read == 2 * p + (uint64_t)side && r.kind != GAP_KIND_NONE;
  }
  if (!ok) atomicMin((unsigned long long *)&a.st[LS_BAD_PAIR], (unsigned long long)p);
}

// the records are valid (kc_depth_check_kernel) and the pairs are (kc_lassm_pair_check_kernel)
template <bool WRITE>
__device__ __forceinline__ void lassm_candidate(const LassmArgs &a, uint32_t end, uint32_t read, uint32_t rc, uint32_t L) {
  if (!WRITE) {
    atomicAdd((unsigned long long *)&a.e_cands[end], 1ull);
    atomicAdd((unsigned long long *)&a.e_bases[end], (unsigned long long)L);
  } else if (a.e_res[end].x > LASSM_TOO_MANY) {
    const uint32_t i = atomicAdd(&a.e_ecur[end], 1u);
    const uint32_t t = atomicAdd(&a.e_tcur[end], L + 1u);
    a.entries[a.e_ent[end] + i] = make_uint4((read << 1) | rc, end, t, L);
  }
}

template <bool WRITE>
__global__ void kc_lassm_cands_kernel(LassmArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n_over = 0, n_mate = 0;
  uint64_t n_bases = 0;
  if (r < a.nreads) {
    const uint32_t L = (uint32_t)(a.offsets[r + 1] - a.offsets[r]);
    const uint4 pr = a.pairs[r >> 1];
    const uint32_t bi = (r & 1) ? pr.y : pr.x, mi = (r & 1) ? pr.x : pr.y;
    if (L && bi != LASSM_NO_ALN) {
      const DepthRec b = depth_load(a.alns, bi);
      const uint32_t u = b.ctg;
      const int64_t len_u = (int64_t)(a.offs[u + 1] - 1u - a.offs[u]);
      const int64_t ps = (int64_t)b.cstart - (int64_t)b.rstart, pe = (int64_t)b.cstop + ((int64_t)L - (int64_t)b.rstop);
      if (pe > len_u) {  // R' hangs over the right end
        lassm_candidate<WRITE>(a, 2u * u + 1u, (uint32_t)r, b.orient, L);
        n_over++;
        n_bases += L;
      }
      if (ps < 0) {  // revcomp(R') hangs over the right end of the reverse complement
        lassm_candidate<WRITE>(a, 2u * u, (uint32_t)r, b.orient ^ 1u, L);
        n_over++;
        n_bases += L;
      }
      const uint64_t m = r ^ 1ull;
      const uint32_t Lm = (uint32_t)(a.offsets[m + 1] - a.offsets[m]);
      bool unplaced = Lm != 0u;
      if (unplaced && mi != LASSM_NO_ALN) unplaced = depth_load(a.alns, mi).ctg != u;
      if (unplaced && b.orient == 0u && ps + (int64_t)a.max_insert > len_u) {
        lassm_candidate<WRITE>(a, 2u * u + 1u, (uint32_t)m, 1u, Lm);
        n_mate++;
        n_bases += Lm;
      }
      if (unplaced && b.orient == 1u && pe - (int64_t)a.max_insert < 0) {
        lassm_candidate<WRITE>(a, 2u * u, (uint32_t)m, 1u, Lm);
        n_mate++;
        n_bases += Lm;
      }
    }
  }
  if (!WRITE) {
    const uint64_t both = wave_sum(((uint64_t)n_mate << 32) | n_over);  // at most 128 each
    n_bases = wave_sum(n_bases);
    if ((threadIdx.x & 63) == 0) {
      if ((uint32_t)both) atomicAdd((unsigned long long *)&a.st[LS_OVERHANG], (unsigned long long)(uint32_t)both);
      if (both >> 32) atomicAdd((unsigned long long *)&a.st[LS_MATE], (unsigned long long)(both >> 32));
      if (n_bases) atomicAdd((unsigned long long *)&a.st[LS_CAND_BASES], (unsigned long long)n_bases);
    }
  }
}

__global__ void kc_lassm_plan_kernel(LassmArgs a) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_ends) return;
  const uint64_t c = a.e_cands[e], b = a.e_bases[e];
  const bool active = c > 0 && c <= (uint64_t)a.max_cands;
  a.e_ent[e] = active ? c : 0ull;
  a.e_text[e] = active ? b + c : 0ull;
  a.e_slots[e] = active ? lassm_slots(b) : 0ull;
  a.e_res[e] = make_uint4(c == 0 ? LASSM_NO_CANDS : active ? LASSM_DEAD_END : LASSM_TOO_MANY, 0u, 0u, 0u);
}

__global__ void kc_lassm_text_kernel(LassmArgs a, uint64_t n_ent) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ent) return;
  const uint4 en = a.entries[i];
  const uint32_t rc = en.x & 1u, L = en.w;
  const uint64_t r0 = a.offsets[en.x >> 1], base = a.e_text[en.y] + en.z;
  uint64_t h = 0;
  for (uint32_t j = 0; j < L; j++) {
    const uint64_t at = r0 + (rc ? L - 1u - j : j);
    uint32_t c = base_code4(a.bases[at]);
    if (rc && c < 4u) c = 3u - c;
    a.tph[base + j] = h;
    a.tcode[base + j] = (uint8_t)(c | (lassm_class(a, at) << 3));
    h = h * LASSM_HASH_BASE + c + 1u;
  }
  a.tph[base + L] = h;
  a.tcode[base + L] = 4;  // the separator: no base, no class
  a.tnb[base + L] = 0;
  uint32_t run = 0;
  for (uint32_t j = L; j-- > 0;) {
    const uint32_t c = base_code4(a.bases[r0 + (rc ? L - 1u - j : j)]);  // a base's complement is a base
    run = c < 4u ? (run < 255u ? run + 1u : 255u) : 0u;
    a.tnb[base + j] = (uint8_t)run;
  }
}

// the m codes at q and at p of one end's text: windows of bases only
// Eight bytes of either a trip, loaded before the first is looked at (a trip is one round trip to memory, not eight); past
// the end the last byte is compared again.
__device__ __forceinline__ bool lassm_same_text(const uint8_t *t, uint64_t q, uint64_t p, uint32_t m) {
  for (uint32_t j = 0; j < m; j += 8) {
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
      const uint32_t at = j + i < m ? j + i : m - 1u;
      diff |= (uint32_t)(t[q + at] ^ t[p + at]);
    }
    if (diff & 7u) return false;
  }
  return true;
}

__global__ void __launch_bounds__(64) kc_lassm_walk_kernel(LassmArgs a, uint32_t e0) {
  __shared__ uint8_t ring[LASSM_MAX_MER];  // code j of S at ring[j & 127]
  const uint32_t lane = threadIdx.x, e = e0 + blockIdx.x;
  if (a.e_res[e].x <= LASSM_TOO_MANY) return;
  const uint32_t u = e >> 1, right = e & 1u;
  const uint32_t o = a.offs[u], len = a.offs[u + 1] - 1u - o;
  const uint32_t tail = len < a.max_mer ? len : a.max_mer;
  uint32_t last_bad = 0;  // 1 + the last position of S that holds no base; the extension adds bases only
  for (uint32_t j0 = 0; j0 < LASSM_MAX_MER; j0 += 64) {
    const uint32_t j = j0 + lane;
    uint32_t c = 0;
    if (j < tail) {
      c = base_code4(right ? a.seqs[o + len - tail + j] : a.seqs[o + tail - 1u - j]);
      if (!right && c < 4u) c = 3u - c;
      ring[j] = (uint8_t)c;
    }
    const uint64_t bad = __ballot(j < tail && c == 4u);
    if (bad) last_bad = j0 + 64u - (uint32_t)__clzll((long long)bad);
  }
  __syncthreads();
  uint64_t thr = a.min_viable;
  if (a.ctgs) {
    const uint64_t t = (uint64_t)a.permille * a.ctgs[2 * (uint64_t)u + 1].w / 1000ull;
    thr = t > thr ? t : thr;
  }
  const uint64_t tlen = a.e_bases[e] + a.e_cands[e], nslots = lassm_slots(a.e_bases[e]);
  const uint32_t mask = (uint32_t)(nslots - 1);
  const uint8_t *tc = a.tcode + a.e_text[e], *tnb = a.tnb + a.e_text[e];
  const uint64_t *tph = a.tph + a.e_text[e];
  uint32_t *tab = a.table + (a.e_slots[e] - a.e_slots[e0]) * LASSM_SLOT_WORDS;
  uint8_t *ext = a.ext + (uint64_t)e * a.max_walk;
  uint32_t m = a.k > a.min_mer ? a.k : a.min_mer;
  m = m < a.max_mer ? m : a.max_mer;
  uint32_t s_len = tail, ext_len = 0, iters = 0, status = LASSM_DEAD_END;
  int last_shift = 0;
  for (;;) {
    iters++;
    for (uint64_t w = lane; w < nslots * LASSM_SLOT_WORDS; w += 64) tab[w] = 0u;
    __threadfence();
    uint64_t bm = 1;  // LASSM_HASH_BASE ^ m
    for (uint32_t j = 0; j < m; j++) bm *= LASSM_HASH_BASE;
    for (uint64_t p0 = 0; p0 < tlen; p0 += 64) {
      const uint64_t p = p0 + lane;
      if (p >= tlen || (uint32_t)tnb[p] <= m) continue;  // m bases and the base behind them: p + m is inside the candidate
      const uint32_t cc = tc[p + m], cls = cc >> 3;
      if (cls == LASSM_CLS_NONE) continue;
      const uint64_t h = tph[p + m] - tph[p] * bm;
      uint32_t slot = lassm_slot(h) & mask;
      for (uint64_t probe = 0; probe < nslots; probe++) {
        uint32_t *s = tab + (uint64_t)slot * LASSM_SLOT_WORDS;
        uint32_t key = lassm_ld(s);
        if (key == 0u) {
          const uint32_t old = atomicCAS(s, 0u, (uint32_t)p + 1u);
          key = old ? old : (uint32_t)p + 1u;
        }
        if (key == (uint32_t)p + 1u || lassm_same_text(tc, key - 1u, p, m)) {
          atomicAdd(s + 2u + (cls == LASSM_CLS_HI ? 0u : 4u) + (cc & 7u), 1u);
          break;
        }
        slot = (slot + 1u) & mask;
      }
    }
    __threadfence();
    status = LASSM_DEAD_END;
    if (s_len >= m && last_bad + m <= s_len) {
      uint64_t h = 0;
      for (uint32_t j = 0; j < m; j++) h = h * LASSM_HASH_BASE + ring[(s_len - m + j) & 127u] + 1u;
      for (;;) {  // a trip appends a base or ends the iteration: at most max_walk - ext_len + 1 trips
        uint32_t slot = lassm_slot(h) & mask;
        bool found = false;
        uint32_t stamp = 0, hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
        for (uint64_t probe = 0; probe < nslots; probe++) {
          // the whole slot at once: its stamp and counters are on their way while the text is compared
          const uint32_t *s = tab + (uint64_t)slot * LASSM_SLOT_WORDS;
          const uint32_t key = lassm_ld(s);
          stamp = lassm_ld(s + 1);
#pragma unroll
          for (uint32_t b = 0; b < 4; b++) {
            hi[b] = lassm_ld(s + 2u + b);
            lo[b] = lassm_ld(s + 6u + b);
          }
          if (key == 0u) break;
          bool ne = false;
          for (uint32_t j = lane; j < m; j += 64) ne = ne || (uint32_t)(tc[(uint64_t)(key - 1u) + j] & 7u) != (uint32_t)ring[(s_len - m + j) & 127u];
          if (!__any(ne ? 1 : 0)) {
            found = true;
            break;
          }
          slot = (slot + 1u) & mask;
        }
        if (!found) break;  // no counts: DEAD_END
        uint32_t *s = tab + (uint64_t)slot * LASSM_SLOT_WORDS;
        // lane 0 wrote every stamp of this iteration, so its own load is the one that counts
        if (lane == 0 && !stamp) __hip_atomic_store(s + 1, iters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t seen = __shfl(stamp, 0);
        if (seen) {
          status = LASSM_LOOP;
          break;
        }
        uint32_t n_viable = 0, vb = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
          if ((uint64_t)hi[b] + lo[b] >= thr && hi[b] >= 1u) {
            n_viable++;
            vb = b;
          }
        }
        if (n_viable == 0u) break;
        if (n_viable >= 2u) {
          status = LASSM_FORK;
          break;
        }
        const uint32_t old = ring[(s_len - m) & 127u];
        __syncthreads();  // every lane has read the ring
        if (lane == 0) {
          ring[s_len & 127u] = (uint8_t)vb;
          ext[ext_len] = (uint8_t)code_letter(vb);
        }
        __syncthreads();
        h = h * LASSM_HASH_BASE + (vb + 1u) - (uint64_t)(old + 1u) * bm;
        s_len++;
        ext_len++;
        if (ext_len == a.max_walk) {
          status = LASSM_MAX_LEN;
          break;
        }
      }
    }
    if (status == LASSM_FORK && last_shift >= 0 && m + a.shift <= a.max_mer) {
      m += a.shift;
      last_shift = 1;
    } else if (status == LASSM_DEAD_END && last_shift <= 0 && m >= a.min_mer + a.shift) {
      m -= a.shift;
      last_shift = -1;
    } else
      break;
  }
  if (lane == 0) a.e_res[e] = make_uint4(status, ext_len, iters, m);
}

__global__ void kc_lassm_lens_kernel(LassmArgs a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t s0 = LASSM_STATUSES, s1 = LASSM_STATUSES, extended = 0;
  uint64_t iters = 0, ext = 0;
  if (u < a.n_ctgs) {
    const uint4 l = a.e_res[2 * (uint64_t)u], r = a.e_res[2 * (uint64_t)u + 1];
    a.newoff[u] = (uint64_t)(a.offs[u + 1] - a.offs[u]) + l.y + r.y;  // the separator is counted
    s0 = l.x;
    s1 = r.x;
    iters = (uint64_t)l.z + r.z;
    ext = (uint64_t)l.y + r.y;
    extended = ext ? 1u : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)LASSM_STATUSES; k++) {
    const uint32_t n = wave_count(s0 == k) + wave_count(s1 == k);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long *)&a.st[LS_STATUS + k], (unsigned long long)n);
  }
  iters = wave_sum(iters);
  ext = wave_sum(ext);
  const uint32_t n_ext = wave_count(extended != 0u);
  if ((threadIdx.x & 63) == 0) {
    if (iters) atomicAdd((unsigned long long *)&a.st[LS_ITERS], (unsigned long long)iters);
    if (ext) atomicAdd((unsigned long long *)&a.st[LS_EXT_BASES], (unsigned long long)ext);
    if (n_ext) atomicAdd((unsigned long long *)&a.st[LS_EXTENDED], (unsigned long long)n_ext);
  }
}

// kc_lassm_end: {u32 cands, ext_len, out_pos; u16 iters; u8 mer_len, status}.  a.newoff is scanned.
__global__ void kc_lassm_ends_kernel(LassmArgs a, uint4 *ends) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_ends) return;
  const uint32_t u = e >> 1;
  const uint4 res = a.e_res[e];
  uint32_t pos = (uint32_t)a.newoff[u];
  if (e & 1u) pos += a.e_res[e - 1u].y + (a.offs[u + 1] - 1u - a.offs[u]);
  ends[e] = make_uint4((uint32_t)a.e_cands[e], res.y, pos, res.z | (res.w << 16) | (res.x << 24));
}

__global__ void kc_lassm_write_kernel(LassmArgs a, uint8_t *out, uint64_t total) {
  const uint64_t j0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (j0 >= total) return;
  uint32_t u = find_le(a.newoff, 0u, a.n_ctgs - 1u, j0);  // the starts increase strictly
  uint64_t start = 0, sep = 0;
  uint32_t xl = 0, len = 0, o = 0;
  auto load = [&]() {
    start = a.newoff[u];
    o = a.offs[u];
    len = a.offs[u + 1] - 1u - o;
    xl = a.e_res[2 * (uint64_t)u].y;
    sep = start + xl + len + a.e_res[2 * (uint64_t)u + 1].y;
  };
  load();
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint64_t j = j0 + (uint64_t)k;
    uint32_t ch = 0;
    if (j < total) {
      const uint64_t t = j - start;
      if (j == sep)
        ch = '_';
      else if (t < xl)  // the left extension, reversed and complemented: the walk wrote one of the four letters there
        ch = base_comp(a.ext[2 * (uint64_t)u * a.max_walk + (xl - 1u - (uint32_t)t)]);
      else if (t < (uint64_t)xl + len)
        ch = a.seqs[o + (uint32_t)(t - xl)];
      else
        ch = a.ext[(2 * (uint64_t)u + 1) * a.max_walk + (uint32_t)(t - xl - len)];
      if (j == sep && u + 1u < a.n_ctgs) {
        u++;
        load();
      }
    }
    w[k >> 2] |= ch << (8 * (k & 3));
  }
  if (j0 + 16 <= total && (((uintptr_t)out) & 15) == 0)
    *(uint4 *)(out + j0) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (j0 + (uint64_t)k < total) out[j0 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}

}  // namespace kc
