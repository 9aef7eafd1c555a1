// kc_dedup.hpp -- duplicate and contained contigs of a seq block (kc_ctg_dedup).  The reference holds no contig code, so the
// rules are this project's own (include/kcount_mi355.h, DESIGN.md section 29, pinned statement by statement by
// tests/dedup_model.py): contig u is redundant iff its text or its reverse complement lies, with at most max_mismatches
// differing bytes, inside a contig that outranks it (longer, or as long and of smaller index).  The seed index of
// kc_align.hpp cannot find that: it throws away exactly the k-mers two copies share.  Here every contig has ONE k-mer, its
// anchor (the first all-ACGT window), and every window of the block is looked up among the anchors.
//
//  kc_dedup_anchor_kernel   a wave per contig: 64 bytes a step, the bad bytes as a ballot, the first run of k good ones;
//                           the anchor's canonical key as kc_align_index_kernel packs it
//  kc_dedup_link_kernel     a thread per anchored contig: into an open-addressing table of 64-bit slots, at most half full.
//                           A slot is a list head -- the key's upper 32 hash bits and a contig + 1 -- and next[u] chains
//                           the contigs that share a key.  List order is free: every result below is an order-free reduction
//  kc_dedup_windows_kernel  a thread per block position, count then write: its window's key probes the table once, key
//                           words are compared (not hashes), the chain is walked with the rank and fit tests.  The count
//                           pass's counters go through wg_stats, an atomic a workgroup of 4096 positions and counter; the
//                           write pass reserves a wave's entries through one cursor.  Candidates of at most DD_LONG bytes
//                           fill the array from its front, longer ones from its back
//  kc_dedup_verify_kernel   the hot path.  A wave per candidate (<false>) or per DD_SEG bytes of a long one (<true>): a
//                           lane owns 16 ALIGNED bytes of the container, the contig's side is two aligned loads and a funnel
//                           shift (shuf_load16), reversed by byte permutes and complemented by bit arithmetic for o = 1.
//                           A wave leaves once it is over max_mismatches; segments add their counts to the candidate's word
//  kc_dedup_best_kernel     per u the greatest (L_v, ~v) over verified candidates, a 64-bit atomicMax
//  kc_dedup_pick_kernel     among those the smallest (j, o) carrying its mismatches, a 64-bit atomicMin
//  kc_dedup_status_kernel   status, absorbed (one atomic a redundant contig), the kept lengths and flags, the statistics
//  kc_dedup_records_kernel  behind the two scans: records, the new offsets, the gather's tables
//  kc_dedup_gather_kernel   output-centric: a lane owns 16 aligned OUTPUT bytes, finds its contig with find_le over the new
//                           offsets and builds the chunk from aligned source loads and a funnel shift; <1> bytes, <2> depths
#pragma once
#include "kc_align.hpp"
#include "kc_common.hpp"
#include "kc_kit.hpp"
#include "kc_shuffle.hpp"

namespace kc {

constexpr int DD_TPB = 256;
constexpr int DD_WIN_TPB = 1024, DD_WIN_ITEMS = 4;  // the windows kernel: 4096 block positions a workgroup
constexpr uint32_t DD_NONE = 0xFFFFFFFFu;
constexpr uint32_t DD_SEG = 8192;    // bytes of a long candidate a wave compares: eight steps of 64 lanes x 16 bytes
constexpr uint32_t DD_LONG = 16384;  // a candidate of more bytes is cut into segments
constexpr uint32_t DD_DUPLICATES_ONLY = 1u, DD_UNANCHORED = 1u;
constexpr uint32_t DD_KEPT = 0, DD_DUPLICATE = 1, DD_CONTAINED = 2;
static_assert(DD_SEG % 1024 == 0 && DD_LONG >= DD_SEG, "a segment is whole wave steps");

enum { DDS_ANCHORED = 0, DDS_WINDOWS, DDS_HITS, DDS_CANDS, DDS_LONG, DDS_MAX_LONG, DDS_CUR_SHORT, DDS_CUR_LONG, DDS_VERIFIED, DDS_DUP, DDS_CONT,
       DDS_KEPT, DDS_REMOVED_BASES, DDS_LONGEST_REMOVED, DDS_KEPT_BYTES, DDS_SCAN_BYTES, DDS_SCAN_KEPT, DDS_COUNT };

struct DedupArgs {
  const uint8_t *seqs;   // the block
  const uint32_t *offs;  // n + 1 starts
  uint32_t nbytes, n;
  int k;
  uint32_t flags, max_mm;
  uint64_t *slots, mask;
  uint64_t *akey;   // NL words a contig: the anchor's canonical key
  uint2 *ainfo;     // x: the anchor's position (DD_NONE: unanchored), y: its forward text is not the canonical one
  uint32_t *next;   // the next contig with the same key
  uint8_t *wflag;   // per DD_WIN_TPB block positions: the count pass found a candidate there, the write pass has work
  uint4 *cands;     // x: u, y: v, z: j, w: o | mismatches << 1
  uint64_t n_cands, n_short, row0;
  uint32_t n_kept, total;  // what stays: contigs and bytes
  uint64_t *best, *pick;  // per contig
  uint32_t *absorbed;
  uint64_t *klen, *kflag, *lbase, *fbase;  // kept bytes and kept flags, scanned in tiles, and the tiles' bases
  uint32_t *noff, *gsrc;                   // per kept contig: its new start (and the total behind the last), its old start
  uint4 *recs;
  uint64_t *offsets_out;
  uint64_t *st;
};

__device__ __forceinline__ uint32_t dd_len(const uint32_t *offs, uint32_t u) { return offs[u + 1] - offs[u] - 1u; }

template <int NL>
__global__ void __launch_bounds__(DD_TPB) kc_dedup_anchor_kernel(DedupArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t u = ((uint64_t)blockIdx.x * DD_TPB + threadIdx.x) >> 6;
  if (u >= a.n) return;  // the whole wave
  const uint32_t s0 = a.offs[u], L = a.offs[u + 1] - s0 - 1u, k = (uint32_t)a.k;
  const uint8_t *t = a.seqs + s0;
  uint32_t run = 0, anchor = DD_NONE;  // run: the position behind the last bad byte
  for (uint32_t c = 0; c < L && anchor == DD_NONE; c += 64) {
    const uint32_t p = c + lane;
    const bool bad = p >= L || !ai_is_acgt_upper(t[p]);
    uint64_t b = __ballot(bad);
    if (b == ~0ull) {  // an N run costs a step for 64 bytes, not a lane's walk
      run = c + 64;
      continue;
    }
    while (b) {
      const uint32_t at = c + (uint32_t)__builtin_ctzll(b);
      if (at - run >= k) {
        anchor = run;
        break;
      }
      run = at + 1;
      b &= b - 1;
    }
    if (anchor == DD_NONE && c + 64 - run >= k) anchor = run;  // good up to the chunk's end, which lies inside the contig
  }
  uint64_t f[NL], r[NL];
  bool swap = false;
  if (anchor != DD_NONE) {
    (void)ai_pack<NL>(t + anchor, a.k, f);
    kc_revcomp<NL>(f, a.k, r);
    swap = kc_less<NL>(r, f);
  }
  if (lane == 0) {
    a.ainfo[u] = make_uint2(anchor, swap ? 1u : 0u);
    if (anchor != DD_NONE) {
#pragma unroll
      for (int j = 0; j < NL; j++) a.akey[u * NL + j] = swap ? r[j] : f[j];
    }
  }
}

template <int NL>
__device__ __forceinline__ bool dd_key_is(const uint64_t *akey, uint32_t u, const uint64_t (&f)[NL]) {
  bool same = true;
#pragma unroll
  for (int j = 0; j < NL; j++) same &= akey[(uint64_t)u * NL + j] == f[j];
  return same;
}

template <int NL>
__global__ void __launch_bounds__(DD_TPB) kc_dedup_link_kernel(DedupArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * DD_TPB + threadIdx.x;
  const uint32_t u = (uint32_t)t;
  const bool anchored = t < a.n && a.ainfo[u].x != DD_NONE;
  wave_add(a.st, DDS_ANCHORED, anchored ? 1ull : 0ull);
  if (!anchored) return;
  uint64_t f[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) f[j] = a.akey[(uint64_t)u * NL + j];
  const uint64_t h = kc_hash<NL>(f), tag = h >> 32, entry = (tag << 32) | (uint64_t)(u + 1u);
  for (uint64_t s = h & a.mask;; s = (s + 1) & a.mask) {  // at most half the slots are ever taken
    uint64_t old = atomicCAS((unsigned long long *)&a.slots[s], 0ULL, (unsigned long long)entry);
    if (old == 0) {
      a.next[u] = DD_NONE;
      return;
    }
    // a head of this key: push in front of it, again where another contig got there first (the new head has the same key)
    while ((old >> 32) == tag && dd_key_is<NL>(a.akey, (uint32_t)old - 1u, f)) {
      a.next[u] = (uint32_t)old - 1u;
      const uint64_t seen = atomicCAS((unsigned long long *)&a.slots[s], (unsigned long long)old, (unsigned long long)entry);
      if (seen == old) return;
      old = seen;
    }
  }
}

// the wave's exclusive prefix sums of c, and their total
__device__ __forceinline__ uint32_t dd_wave_excl(uint32_t c, int lane, uint32_t &total) {
  uint32_t incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  total = __shfl(incl, 63);
  return incl - c;
}

// One block position: its window's key probes the table, the chain of the contigs with that key is walked.  Count pass: adds
// to mine (windows, hits, candidates, long candidates) and to longest.  Write pass: the wave's candidates go to the array,
// reserved through one cursor a wave (every lane of the wave calls this).
template <int NL, bool WRITE>
__device__ __forceinline__ void dd_window(const DedupArgs &a, uint64_t p, int lane, uint32_t (&mine)[4], uint32_t &longest) {
  const uint32_t k = (uint32_t)a.k;
  uint64_t f[NL], r[NL];
  bool window = p + k <= a.nbytes;
  if (window) window = ai_pack<NL>(a.seqs + p, a.k, f);  // a '_' is no base: a window never crosses one
  uint32_t head = DD_NONE;
  bool wswap = false, pal = false;
  if (window) {
    kc_revcomp<NL>(f, a.k, r);
    wswap = kc_less<NL>(r, f);
    pal = ai_equal<NL>(f, r);
    if (wswap) {
#pragma unroll
      for (int j = 0; j < NL; j++) f[j] = r[j];
    }
    const uint64_t h = kc_hash<NL>(f), tag = h >> 32;
    for (uint64_t s = h & a.mask;; s = (s + 1) & a.mask) {
      const uint64_t e = a.slots[s];
      if (e == 0) break;
      if ((e >> 32) != tag) continue;
      if (dd_key_is<NL>(a.akey, (uint32_t)e - 1u, f)) {
        head = (uint32_t)e - 1u;
        break;
      }
    }
  }
  uint32_t v = 0, w = 0, lv = 0;
  if (head != DD_NONE) {
    v = find_le(a.offs, 0u, a.n - 1u, (uint32_t)p);
    w = (uint32_t)p - a.offs[v];
    lv = dd_len(a.offs, v);
  }
  // the candidates of this window: emit(u, j, o, L_u)
  auto walk = [&](auto &&emit) {
    for (uint32_t u = head; u != DD_NONE; u = a.next[u]) {
      if (u == v) continue;
      const uint32_t lu = dd_len(a.offs, u);
      if (!(lv > lu || (lv == lu && v < u))) continue;
      if ((a.flags & DD_DUPLICATES_ONLY) && lv != lu) continue;
      const uint2 ai = a.ainfo[u];
      const uint32_t need = wswap == (ai.y != 0u) ? 0u : 1u;  // the forward texts agree, or one is the other's reverse complement
      for (uint32_t o = 0; o < 2; o++) {
        if (!pal && o != need) continue;
        const int64_t j = (int64_t)w - (int64_t)(o ? lu - k - ai.x : ai.x);
        if (j < 0 || j + (int64_t)lu > (int64_t)lv) continue;
        emit(u, (uint32_t)j, o, lu);
      }
    }
  };
  uint32_t cs = 0, cl = 0;
  walk([&](uint32_t, uint32_t, uint32_t, uint32_t lu) {
    if (lu > DD_LONG) {
      cl++;
      longest = lu > longest ? lu : longest;
    } else
      cs++;
  });
  if (!WRITE) {
    mine[0] += window ? 1u : 0u;
    mine[1] += head != DD_NONE ? 1u : 0u;
    mine[2] += cs + cl;
    mine[3] += cl;
    if (cs + cl) a.wflag[p / DD_WIN_TPB] = 1;  // every writer stores the same
  } else {
    uint32_t ts, tl;
    const uint32_t es = dd_wave_excl(cs, lane, ts), el = dd_wave_excl(cl, lane, tl);
    if (ts + tl == 0) return;  // the whole wave
    unsigned long long bs = 0, bl = 0;
    if (lane == 0) {
      if (ts) bs = atomicAdd((unsigned long long *)&a.st[DDS_CUR_SHORT], (unsigned long long)ts);
      if (tl) bl = atomicAdd((unsigned long long *)&a.st[DDS_CUR_LONG], (unsigned long long)tl);
    }
    bs = __shfl(bs, 0);
    bl = __shfl(bl, 0);
    uint64_t is = bs + es, il = bl + el;
    walk([&](uint32_t u, uint32_t j, uint32_t o, uint32_t lu) {
      const uint64_t at = lu > DD_LONG ? a.n_cands - 1 - il++ : is++;
      if (at < a.n_cands) a.cands[at] = make_uint4(u, v, j, o);  // always: the count pass counted the same candidates
    });
  }
}

// A workgroup of the count pass takes DD_WIN_ITEMS x DD_WIN_TPB positions, a thread one of every DD_WIN_TPB, and its four
// counters go through wg_stats, one atomic a workgroup and counter: a wave's atomic for every 64 positions made the count
// pass eight times the write pass.  The write pass has no counters and takes DD_WIN_TPB positions, and
// only those in which the count pass met a candidate.
template <int NL, bool WRITE>
__global__ void __launch_bounds__(DD_WIN_TPB) kc_dedup_windows_kernel(DedupArgs a) {
  constexpr int ITEMS = WRITE ? 1 : DD_WIN_ITEMS;
  if (WRITE && !a.wflag[blockIdx.x]) return;  // the whole workgroup: candidates are few, most of the block has none
  const int lane = threadIdx.x & 63;
  uint32_t mine[4] = {0u, 0u, 0u, 0u}, longest = 0;
#pragma unroll 1
  for (int i = 0; i < ITEMS; i++)
    dd_window<NL, WRITE>(a, ((uint64_t)blockIdx.x * ITEMS + i) * DD_WIN_TPB + threadIdx.x, lane, mine, longest);
  if (!WRITE) {
    longest = wave_max(longest);
    if (lane == 0 && longest) atomicMax((unsigned long long *)&a.st[DDS_MAX_LONG], (unsigned long long)longest);
    const int k[4] = {DDS_WINDOWS, DDS_HITS, DDS_CANDS, DDS_LONG};
    wg_stats<4>(a.st, k, mine);
  }
}

// the complement of sixteen block bytes, four a word: A <-> T differ in 0x15, C <-> G in 0x04, N stays.  Bit 1 is set in C G N,
// bit 3 in N alone
__device__ __forceinline__ uint32_t dd_comp4(uint32_t x) {
  const uint32_t b1 = (x >> 1) & 0x01010101u, b3 = (x >> 3) & 0x01010101u;
  const uint32_t cg = b1 & ~b3, at = b1 ^ 0x01010101u;
  return x ^ ((cg << 2) | (at * 0x15u));
}

// the bytes of x that are not zero
__device__ __forceinline__ uint32_t dd_nonzero_bytes(uint32_t x) {
  return (uint32_t)__popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

// LONG: blockIdx.y + row0 is the long candidate (they fill the array from its back), the wave of the row its segment
template <bool LONG>
__global__ void __launch_bounds__(DD_TPB) kc_dedup_verify_kernel(DedupArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * DD_TPB + threadIdx.x) >> 6;
  const uint64_t ci = LONG ? a.n_short + a.row0 + blockIdx.y : wave;
  if (ci >= (LONG ? a.n_cands : a.n_short)) return;  // the whole wave
  const uint4 cd = a.cands[ci];
  const uint32_t u = cd.x, v = cd.y, o = cd.w & 1u;
  const uint32_t su = a.offs[u], lu = a.offs[u + 1] - su - 1u;
  const uintptr_t lo = (uintptr_t)a.seqs, hi = lo + a.nbytes;
  const uintptr_t va = lo + a.offs[v] + cd.z;  // the container's byte against (o ? rc(T_u) : T_u)[0]
  const uint32_t mis = (uint32_t)(va & 15u);
  // chunk t is the container's aligned sixteen bytes at va - mis + 16 t: the contig's bytes i in [16 t - mis, 16 t - mis + 16)
  const uint64_t nchunks = ((uint64_t)lu + mis + 15) / 16;
  uint64_t t0 = 0, t1 = nchunks;
  if (LONG) {
    t0 = wave * (DD_SEG / 16);
    if (t0 >= nchunks) return;
    t1 = t0 + DD_SEG / 16 < nchunks ? t0 + DD_SEG / 16 : nchunks;
    if ((cd.w >> 1) > a.max_mm) return;  // other segments are over the limit already
  }
  uint32_t mm = 0;
  for (uint64_t tb = t0; tb < t1; tb += 64) {
    const uint64_t t = tb + lane;
    uint32_t step = 0;
    if (t < t1) {
      const int64_t ia = (int64_t)(16 * t) - (int64_t)mis;
      const uintptr_t aa = va - mis + 16 * t;
      const bool whole = ia >= 0 && ia + 16 <= (int64_t)lu && aa >= lo && aa + 16 <= hi;
      uint32_t wb[4];
      // o = 1: rc(T_u)[ia .. ia + 15] are T_u's bytes lu - 16 - ia .. lu - 1 - ia, backwards and complemented
      if (whole && shuf_load16(lo, hi, lo + su + (o ? (uintptr_t)(lu - 16u) - (uintptr_t)ia : (uintptr_t)ia), wb)) {
        const uint4 x = *(const uint4 *)aa;
        if (o) {
          const uint32_t r0 = dd_comp4(__builtin_bswap32(wb[3])), r1 = dd_comp4(__builtin_bswap32(wb[2]));
          const uint32_t r2 = dd_comp4(__builtin_bswap32(wb[1])), r3 = dd_comp4(__builtin_bswap32(wb[0]));
          wb[0] = r0, wb[1] = r1, wb[2] = r2, wb[3] = r3;
        }
        step = dd_nonzero_bytes(x.x ^ wb[0]) + dd_nonzero_bytes(x.y ^ wb[1]) + dd_nonzero_bytes(x.z ^ wb[2]) + dd_nonzero_bytes(x.w ^ wb[3]);
      } else {  // a candidate's first and last chunk, or aligned loads that would leave the block
        const int64_t from = ia < 0 ? 0 : ia, to = ia + 16 < (int64_t)lu ? ia + 16 : (int64_t)lu;
        for (int64_t i = from; i < to; i++) {
          const uint32_t x = *(const uint8_t *)(va + i);
          const uint32_t y = o ? base_comp(a.seqs[su + lu - 1u - (uint32_t)i]) : a.seqs[su + (uint32_t)i];
          step += x != y ? 1u : 0u;
        }
      }
    }
    mm += step;
    if (__ballot(step != 0u)) {  // the whole wave: over the limit, the rest is not read
      if (wave_sum(mm) > a.max_mm) break;
    }
  }
  mm = wave_sum(mm);
  if (lane == 0) {
    uint32_t *word = (uint32_t *)&a.cands[ci] + 3;
    if (LONG) {
      if (mm) atomicAdd(word, mm << 1);  // at most lu < 2^31 over all segments
    } else
      *word = o | (mm << 1);
  }
}

__device__ __forceinline__ uint64_t dd_rank_key(uint32_t lv, uint32_t v) { return ((uint64_t)lv << 32) | (uint64_t)(~v); }

__global__ void __launch_bounds__(DD_TPB) kc_dedup_best_kernel(DedupArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * DD_TPB + threadIdx.x;
  bool ok = false;
  if (i < a.n_cands) {
    const uint4 cd = a.cands[i];
    ok = (cd.w >> 1) <= a.max_mm;
    if (ok) atomicMax((unsigned long long *)&a.best[cd.x], (unsigned long long)dd_rank_key(dd_len(a.offs, cd.y), cd.y));
  }
  wave_add(a.st, DDS_VERIFIED, ok ? 1ull : 0ull);
}

__global__ void __launch_bounds__(DD_TPB) kc_dedup_pick_kernel(DedupArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * DD_TPB + threadIdx.x;
  if (i >= a.n_cands) return;
  const uint4 cd = a.cands[i];
  if ((cd.w >> 1) > a.max_mm || a.best[cd.x] != dd_rank_key(dd_len(a.offs, cd.y), cd.y)) return;
  // j < 2^31: (j, o, mismatches) in 31 + 1 + 32 bits
  atomicMin((unsigned long long *)&a.pick[cd.x], ((unsigned long long)cd.z << 33) | ((unsigned long long)(cd.w & 1u) << 32) | (cd.w >> 1));
}

__global__ void __launch_bounds__(DD_TPB) kc_dedup_status_kernel(DedupArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * DD_TPB + threadIdx.x;
  const uint32_t u = (uint32_t)t;
  uint32_t dup = 0, cont = 0, kept = 0, gone = 0, stays = 0;
  if (t < a.n) {
    const uint32_t lu = dd_len(a.offs, u);
    const uint64_t b = a.best[u];
    if (b) {
      atomicAdd(&a.absorbed[~(uint32_t)b], 1u);
      dup = (uint32_t)(b >> 32) == lu ? 1u : 0u;
      cont = dup ^ 1u;
      gone = lu;
    } else {
      kept = 1u;
      stays = lu + 1u;
    }
    a.klen[u] = stays;
    a.kflag[u] = kept;
  }
  // a workgroup's removed bases may pass 32 bits (256 contigs of 2^30): the byte sums go a wave at a time
  wave_add(a.st, DDS_REMOVED_BASES, (unsigned long long)gone);
  wave_add(a.st, DDS_KEPT_BYTES, (unsigned long long)stays);
  gone = wave_max(gone);
  if ((threadIdx.x & 63) == 0 && gone) atomicMax((unsigned long long *)&a.st[DDS_LONGEST_REMOVED], (unsigned long long)gone);
  const int k[3] = {DDS_DUP, DDS_CONT, DDS_KEPT};
  const uint32_t mine[3] = {dup, cont, kept};
  wg_stats<3>(a.st, k, mine);
}

// klen, kflag: scanned in tiles; n_kept contigs and total bytes are kept (n >= 1, so both are at least 1)
__global__ void __launch_bounds__(DD_TPB) kc_dedup_records_kernel(DedupArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * DD_TPB + threadIdx.x;
  if (t >= a.n) return;
  const uint32_t u = (uint32_t)t, lu = dd_len(a.offs, u);
  const uint64_t b = a.best[u];
  const uint32_t at = (uint32_t)(a.lbase[t >> LINK_SCAN_SHIFT] + a.klen[u]), idx = (uint32_t)(a.fbase[t >> LINK_SCAN_SHIFT] + a.kflag[u]);
  if (!b) {
    a.noff[idx] = at;
    a.gsrc[idx] = a.offs[u];
    if (a.offsets_out) a.offsets_out[idx] = at;
  }
  if (u == 0) {
    a.noff[a.n_kept] = a.total;
    if (a.offsets_out) a.offsets_out[a.n_kept] = a.total;
  }
  if (a.recs) {
    const uint64_t pk = a.pick[u];
    const uint32_t lv = (uint32_t)(b >> 32), unanchored = a.ainfo[u].x == DD_NONE ? DD_UNANCHORED : 0u;
    const uint32_t orient = b ? (uint32_t)(pk >> 32) & 1u : 0u;
    a.recs[2 * t] = make_uint4(!b ? DD_KEPT : lv == lu ? DD_DUPLICATE : DD_CONTAINED, b ? ~(uint32_t)b : DD_NONE, b ? (uint32_t)(pk >> 33) : 0u,
                               b ? (uint32_t)pk : 0u);
    a.recs[2 * t + 1] = make_uint4(b ? DD_NONE : idx, lu, a.absorbed[u], orient | (unanchored << 8));
  }
}

struct DedupCopy {
  const uint8_t *src;  // elements of ES bytes
  uint8_t *dst;
  const uint32_t *noff, *gsrc;  // in elements
  uint32_t n_kept, total, src_total;
};

// Thread t owns dst's bytes [16 t - mis, 16 t - mis + 16) cut to [0, ES total): mis = dst's address & 15, so every whole chunk
// is an aligned 16-byte store.  n_kept >= 1 and total >= 1 (the host launches nothing otherwise); ES = 2: dst is 2-byte aligned.
template <int ES>
__global__ void __launch_bounds__(DD_TPB) kc_dedup_gather_kernel(DedupCopy a) {
  const int64_t mis = (int64_t)((uintptr_t)a.dst & 15u), tb = (int64_t)ES * a.total;
  const int64_t p0 = (int64_t)(((uint64_t)blockIdx.x * DD_TPB + threadIdx.x) * 16) - mis;
  if (p0 >= tb) return;
  const int64_t from = p0 < 0 ? 0 : p0, to = p0 + 16 < tb ? p0 + 16 : tb;
  uint32_t q = find_le(a.noff, 0u, a.n_kept - 1u, (uint32_t)(from / ES));  // noff[0] = 0
  int64_t qs = (int64_t)ES * a.noff[q], qe = (int64_t)ES * a.noff[q + 1], sp = (int64_t)ES * a.gsrc[q];
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const bool whole = to - from == 16;
  const uintptr_t src_lo = (uintptr_t)a.src, src_hi = src_lo + (uintptr_t)ES * a.src_total;
  bool done = false;
  if (whole && to <= qe)
    done = shuf_load16(src_lo, src_hi, src_lo + (uintptr_t)(sp + (from - qs)), w);
  else if (whole && q + 1 < a.n_kept && to <= (int64_t)ES * a.noff[q + 2]) {
    // two contigs: `cut` bytes (1 .. 15: the search gave the contig that holds `from`) end contig q, the others begin contig
    // q + 1; either comes out of sixteen bytes loaded from where the chunk would lie in that contig's source
    const uint32_t cut = (uint32_t)(qe - from);
    uint32_t v[4];
    done = shuf_load16(src_lo, src_hi, src_lo + (uintptr_t)(sp + (from - qs)), w) &&
           shuf_load16(src_lo, src_hi, src_lo + (uintptr_t)((int64_t)ES * a.gsrc[q + 1]) - cut, v);
    if (done) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t nb = cut > 4u * j ? cut - 4u * j : 0u;  // bytes of word j that are contig q's
        const uint32_t m = nb >= 4u ? 0xFFFFFFFFu : (1u << (8u * nb)) - 1u;
        w[j] = (w[j] & m) | (v[j] & ~m);
      }
    }
  }
  if (!done) {  // an end of the block, a chunk over three contigs or more, or aligned loads that would leave the source array
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      uint32_t c = 0;
      if (p >= from && p < to) {
        while (p >= qe) {  // ends: noff[n_kept] = total
          q++;
          qs = qe;
          qe = (int64_t)ES * a.noff[q + 1];
          sp = (int64_t)ES * a.gsrc[q];
        }
        c = a.src[sp + (p - qs)];
      }
      w[j >> 2] |= c << (8 * (j & 3));
    }
  }
  if (whole)
    *(uint4 *)(a.dst + p0) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t p = p0 + j;
      if (p >= from && p < to) a.dst[p] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

}  // namespace kc
