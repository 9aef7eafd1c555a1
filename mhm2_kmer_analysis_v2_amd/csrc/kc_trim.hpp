// kc_trim.hpp -- adapter trimming on the device (kc_adapters_load, kc_trim_adapters): the reference's Adapters::trim
// and trim_pair (src/adapters.cpp:171-273) in the build it ships, MERGE_READS_TRIM_WITH_SSW (CMakeDefinitions.txt:48),
// the step merge_reads runs in front of its pair loop (src/merge_reads.cpp:469) and PackedReads::load_reads_nb per
// read (src/packed_reads.cpp:386-390).
//
// Rules (the contract of the kernels below and of tests/trim_model.py):
//  * Loading (Adapters::load_adapter_seqs, src/adapters.cpp:48-146): the FASTA text line by line as getline yields it;
//    a line whose first byte is '>' is a name, any other line a sequence; a sequence shorter than adapter_k (an empty
//    line too) is ignored and counted; a trailing CR is not stripped.  Every kept sequence s becomes the entries s
//    (index 2n) and revcomp(s) (index 2n+1); revcomp is src/utils.cpp:98-129 (IUPAC -> N, lower -> upper case, any
//    other byte KC_ERR_BAD_BASE where the reference DIEs -- a CR among them).  Every k-mer of every entry is indexed
//    (Kmer<32>::get_kmers with check_n = false, src/kmer.cpp:156-192): the 2-bit code of a byte c is
//    x = (c & 4) >> 1, code = x + ((x ^ (c & 2)) >> 1), so N counts as G, no k-mer is invalid and the case does not
//    matter; k-mers are not canonicalised.  A k-mer maps to its (entry, offset) records in insertion order, entry
//    ascending, then offset ascending.  adapter_k <= 32 (MAX_ADAPTER_K, src/adapters.hpp:56).
//  * One read (Adapters::trim, :171-258): a read shorter than adapter_k is left alone.  The read's k-mers (same code)
//    are visited at i = 0, 4, 8, ... (STEP, :183).  For a k-mer in the index the records are walked in order; one
//    whose entry was already aligned for this read is skipped, the first one whose entry was not is aligned, and the
//    walk of that k-mer ends (:240).  The alignment (:201-207): start = max(0, offset - i - 2),
//    len = min(start + read_len + 2, adapter_len), query = adapter.substr(start, len), reference = the whole read as
//    it came.  max_match_len = min(adapter_len, read_len - ref_begin) in size_t arithmetic (ref_begin = -1 gives
//    read_len + 1), identity = (double)score / (double)match_score / (double)max_match_len; identity >=
//    best_identity takes over best_trim_pos = ref_begin; identity > 0.97 ends the scan.  Afterwards (:247-256), with
//    best_identity >= 0.5: a best_trim_pos < 12 becomes 0, the read and its qualities are cut to best_trim_pos,
//    reads_removed counts cuts to 0, bases_trimmed sums the bases cut, and the read counts as trimmed even when
//    nothing was cut.
//  * Scores, match / mismatch / gap open / gap extend / ambiguity: 1,1,1,1,1 (ALTERNATE_ALN_SCORES), or 2,3,5,2,1
//    (BLASTN_ALN_SCORES, CMakeDefinitions.txt:133-134; Aligner::ReBuild(string), src/ssw/ssw.cpp:468-480).  Bytes are
//    translated by kBaseTranslation (src/ssw/ssw.cpp:13-23): A C G T in either case 0-3, U and u 0, everything else 4;
//    a 4 on either side scores -ambiguity (BuildSwScoreMatrix, :25-49).
//  * The aligner (ssw_align with flag 0x08, src/ssw/ssw_core.cpp:200-403, 874-955) yields score1 and ref_begin1.  Its
//    values are those of the affine-gap local alignment H = max(0, diag + s, E, F), a gap of n costing
//    open + (n - 1) * extend, in exact integers.  E of the next column is taken from H before F's correction (:295);
//    with these scores that changes no H, because a gap down a column next to a gap along a row is never better than
//    a substitution with both gaps one shorter, and for the same reason F may be taken from the uncorrected H of the
//    rows above.  The byte lanes give way to word lanes once max + bias >= 255 (:338, :898-901); both equal the
//    exact integers (tests/golden/ssw_ref_alignments.json crosses that line both ways).  One exception is not
//    reproduced: with equal gap open and extend penalties (1,1,1,1,1) the word lanes' lazy-F loop stops after one
//    row, which can only show for scores of 254 and more, i.e. adapters of 254 bases and more.
//    Ties: the ending column is the first column in scan order whose maximum is strictly greater than every earlier
//    one (:336), the ending row the smallest query index holding the maximum in that column (:358-368).  The
//    beginning comes from a second pass over the reversed query prefix [0, query_end] against the reference from
//    ref_end downwards, which stops at the first column whose maximum equals score1 (:352); ref_begin1 is that pass's
//    ending column, -1 when the score is 0.
//  * Pairs (Adapters::trim_pair, :260-273): both mates are trimmed; if either counted as trimmed and both are then
//    longer than 1, both are cut to the shorter length.
//  * Limits: a read longer than 32767 is KC_ERR_INVALID_ARG (kc_merge_pairs' limit), an entry longer than
//    TR_MAX_ENTRY_LEN or more than TR_MAX_ENTRIES entries are KC_ERR_INVALID_ARG at load time.  Base and quality bytes
//    are not validated: the reference's trim looks at no quality, and any byte has a k-mer code and an SSW code.
//
// Kernels:
//  kc_trim_seed_kernel   a wave takes TR_RPW reads, one at a time: lane t loads bases 4t .. 4t+3 as one word, turns them
//                        into four 2-bit codes in one byte, three shuffles gather the eight bytes from lane t on (the
//                        k-mer at 4t), one probe of the k-mer table.  Almost every read of clean data leaves here:
//                        its length is stored, nothing else.  A read with a hit goes to a list.
//  kc_trim_align_kernel  a wave per listed read walks its hits in order (the scan is sequential: which entry is
//                        aligned depends on those aligned before).  An alignment lays a column of the matrix across
//                        the lanes, R rows a lane; the F dependency down the column is a prefix maximum over the wave
//                        (F(j) = max over j' < j of H'(j') + j' * extend, less open + (j - 1) * extend), not a lazy
//                        loop.  Both passes run in the same wave; the read's bytes come 64 columns at a time and are
//                        broadcast from registers, so any read length takes the same path.
//  kc_trim_sizes_kernel  final lengths (the pair rule) and per-tile byte sums; kc_scan_kernel<1> (kc_scan.hpp) scans them.
//  kc_trim_write_kernel  a workgroup per tile: in-tile offsets, then bases, qualities and offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kc_merge.hpp"

namespace kc {

constexpr int TR_STEP = 4;                 // src/adapters.cpp:183
constexpr int TR_MIN_TRIM_POS = 12;        // :248
constexpr int TR_MAX_K = 32;               // MAX_ADAPTER_K
constexpr int TR_MAX_ENTRY_LEN = 1024;     // rows of the widest alignment: 16 a lane
constexpr int TR_MAX_ENTRIES = 65536;      // bits of the align kernel's "already aligned" set in LDS
constexpr int TR_REC_OFF_BITS = 10;        // a record: entry << 10 | offset
constexpr int TR_RPW = 32;                 // reads per wave of the seed kernel
constexpr int TR_SEED_WAVES = 4;
constexpr int TR_CHUNK = 56;               // seed positions per round: lane t needs the bytes of lanes t .. t + 7
constexpr int TR_TILE = 256;               // reads per workgroup of the size and write kernels
constexpr uint32_t TR_RES_TRIMMED = 1u << 31;

enum { TRS_TRIMMED = 0, TRS_BASES, TRS_REMOVED, TRS_ALIGN, TRS_N };
enum { TR_CTL_ERR = 0, TR_CTL_NLIST, TR_CTL_N };

struct TrSlot {
  uint64_t key;
  uint32_t rec_start, rec_count;  // rec_count 0: empty
};

struct TrimArgs {
  const uint8_t *bases, *quals;
  const uint64_t *offsets;
  uint64_t nreads;
  int k, paired;
  int match, mismatch, gap_open, gap_ext, amb;
  // the adapter set
  const TrSlot *slots;
  uint32_t slot_mask, lg_slots;
  const uint32_t *recs;
  const uint32_t *ent_off;  // [n_entries + 1]
  const uint8_t *ent_bytes;
  uint32_t n_entries;
  // scratch
  uint32_t *res;    // [nreads] length after trim | TR_RES_TRIMMED
  uint32_t *flen;   // [nreads] final length (pair rule applied)
  uint32_t *list;   // [nreads] reads with a seed hit
  uint64_t *tile_bytes;
  unsigned long long *stats;  // [TRS_N]
  uint32_t *ctl;              // [TR_CTL_N]
  uint8_t *out_bases, *out_quals;
  uint64_t *out_offsets;
};

// the 2-bit code of Kmer::get_kmers, src/kmer.cpp:191-192
__host__ __device__ __forceinline__ uint32_t tr_kcode(uint32_t c) {
  const uint32_t x = (c & 4u) >> 1;
  return x + ((x ^ (c & 2u)) >> 1);
}

// kBaseTranslation, src/ssw/ssw.cpp:13-23
__host__ __device__ __forceinline__ int tr_ssw_code(uint32_t c) {
  const uint32_t u = c & 0xDFu;
  return u == 'A' || u == 'U' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

__host__ __device__ __forceinline__ uint32_t tr_hash(uint64_t key, uint32_t lg) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - lg));
}

// the records of a k-mer: rec_count (0: not in the index) and rec_start
__device__ __forceinline__ uint32_t tr_lookup(const TrimArgs &a, uint64_t key, uint32_t &rec_start) {
  uint32_t s = tr_hash(key, a.lg_slots);
  for (;;) {
    const TrSlot sl = a.slots[s];
    if (!sl.rec_count) return 0;
    if (sl.key == key) {
      rec_start = sl.rec_start;
      return sl.rec_count;
    }
    s = (s + 1) & a.slot_mask;
  }
}

__device__ __forceinline__ uint64_t tr_kmask(int k) { return k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull; }

// the k-mers at the positions 4 * (c0 + lane), lane < TR_CHUNK, of the read at `off` of `len` bases: the key (base p
// of the k-mer in bits 2p, 2p+1), or no k-mer there.  end: the bytes of the whole input.
__device__ __forceinline__ bool tr_seed_keys(const uint8_t *bases, uint64_t off, int len, int c0, int lane, int k, uint64_t end,
                                             uint64_t &key) {
  const int i = TR_STEP * (c0 + lane);
  uint32_t d = 0;
  if (i < len) {
    const uint64_t at = off + (uint64_t)i;
    if (at + 4 <= end) {
      __builtin_memcpy(&d, bases + at, 4);
    } else {
      for (uint64_t b = 0; at + b < end; b++) d |= (uint32_t)bases[at + b] << (8 * b);
    }
  }
  const uint32_t x = (d & 0x04040404u) >> 1;
  const uint32_t cd = x + ((x ^ (d & 0x02020202u)) >> 1);  // four codes, one a byte
  const uint32_t pb = (cd | (cd >> 6) | (cd >> 12) | (cd >> 18)) & 0xFFu;
  const uint32_t w1 = pb | ((uint32_t)__shfl_down((int)pb, 1) << 8);
  const uint32_t w2 = w1 | ((uint32_t)__shfl_down((int)w1, 2) << 16);
  const uint64_t w3 = (uint64_t)w2 | ((uint64_t)(uint32_t)__shfl_down((int)w2, 4) << 32);
  key = w3 & tr_kmask(k);
  return lane < TR_CHUNK && i + k <= len;
}

__global__ void __launch_bounds__(64 * TR_SEED_WAVES) kc_trim_seed_kernel(TrimArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t r0 = ((uint64_t)blockIdx.x * TR_SEED_WAVES + wv) * TR_RPW;
  if (r0 >= a.nreads) return;
  const uint64_t end = a.offsets[a.nreads];
  const int nr = a.nreads - r0 < (uint64_t)TR_RPW ? (int)(a.nreads - r0) : TR_RPW;
  const uint64_t myoff = lane <= nr ? a.offsets[r0 + lane] : 0;
  const uint64_t nxt = __shfl_down(myoff, 1);
  const uint64_t mylen = nxt - myoff;  // lanes < nr
  bool bad = lane < nr && (nxt < myoff || mylen > (uint64_t)MG_MAX_LEN);
  if (__ballot(bad)) {
    if (lane == 0) atomicOr(&a.ctl[TR_CTL_ERR], 1u);
    return;
  }
  uint64_t hits = 0;  // reads of this wave with a k-mer in the index
  for (int j = 0; j < nr; j++) {
    const uint64_t off = __shfl(myoff, j);
    const int len = (int)__shfl(mylen, j);
    bool hit = false;
    for (int c0 = 0; TR_STEP * c0 + a.k <= len; c0 += TR_CHUNK) {
      uint64_t key;
      uint32_t rs;
      if (tr_seed_keys(a.bases, off, len, c0, lane, a.k, end, key)) hit |= tr_lookup(a, key, rs) != 0;
    }
    if (__ballot(hit)) hits |= 1ull << j;
  }
  if (lane < nr) a.res[r0 + lane] = (uint32_t)mylen;
  if (hits) {
    const int n = __popcll(hits);
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&a.ctl[TR_CTL_NLIST], (uint32_t)n);
    base = __shfl(base, 0);
    if ((hits >> lane) & 1ull) a.list[base + __popcll(hits & ((1ull << lane) - 1ull))] = (uint32_t)(r0 + lane);
  }
}

struct TrAln {
  int score, end_col, end_row;
};

constexpr int TR_NEG = -(1 << 28);

// One pass of the aligner.  Query row j is q[j * qstep], j < qn, lane l holding rows l * R .. l * R + R - 1; column c is
// ref[c * rstep], c < rn, in scan order.  term: stop at the first column holding that score (-1: never).  Wave-uniform
// result: the best score, its first column (-1: score 0) and the smallest row holding it there.
template <int R>
__device__ __forceinline__ TrAln tr_sw_pass(const TrimArgs &a, const uint8_t *q, int qstep, int qn, const uint8_t *ref, int rstep, int rn,
                                            int term, int lane) {
  int H[R], E[R], qc[R];
#pragma unroll
  for (int t = 0; t < R; t++) {
    const int row = lane * R + t;
    qc[t] = row < qn ? tr_ssw_code(q[(long)row * qstep]) : 4;
    H[t] = E[t] = 0;
  }
  const int go = a.gap_open, ge = a.gap_ext;
  int lbest = 0, lkey = 0x7FFFFFFF;
  bool done = false;
  for (int c0 = 0; c0 < rn && !done; c0 += 64) {
    const int ci = c0 + lane;
    const int cr = ci < rn ? tr_ssw_code(ref[(long)ci * rstep]) : 4;
    const int cnt = rn - c0 < 64 ? rn - c0 : 64;
    for (int c = 0; c < cnt; c++) {
      const int r = __shfl(cr, c);
      int prev = __shfl_up(H[R - 1], 1);
      if (lane == 0) prev = 0;
      int hp[R], pre[R];
      int loc = TR_NEG;
#pragma unroll
      for (int t = 0; t < R; t++) {
        const int s = (r == 4 || qc[t] == 4) ? -a.amb : (r == qc[t] ? a.match : -a.mismatch);
        const int d = prev + s;
        prev = H[t];
        int h = d > E[t] ? d : E[t];
        h = h > 0 ? h : 0;
        hp[t] = h;
        pre[t] = loc;
        const int av = h + (lane * R + t) * ge;
        loc = loc > av ? loc : av;
      }
      int inc = loc;  // inclusive prefix maximum over the lanes
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const int v = __shfl_up(inc, s);
        if (lane >= s) inc = inc > v ? inc : v;
      }
      int ex = __shfl_up(inc, 1);
      if (lane == 0) ex = TR_NEG;
      bool hit = false;
#pragma unroll
      for (int t = 0; t < R; t++) {
        const int row = lane * R + t;
        const int run = ex > pre[t] ? ex : pre[t];
        const int f = run - go - (row - 1) * ge;
        const int h = hp[t] > f ? hp[t] : f;
        H[t] = h;
        const int e1 = E[t] - ge, e2 = hp[t] - go;  // ssw_core.cpp:295: from H before F's correction
        E[t] = e1 > e2 ? e1 : e2;
        if (row < qn) {
          if (h > lbest) {
            lbest = h;
            lkey = ((c0 + c) << 16) | row;
          }
          hit |= h == term;
        }
      }
      if (term > 0 && __ballot(hit)) {
        done = true;
        break;
      }
    }
  }
  int best = lbest;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int v = __shfl_xor(best, s);
    best = best > v ? best : v;
  }
  int key = (lbest == best && best > 0) ? lkey : 0x7FFFFFFF;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int v = __shfl_xor(key, s);
    key = key < v ? key : v;
  }
  TrAln o;
  o.score = best;
  o.end_col = best > 0 ? key >> 16 : -1;
  o.end_row = best > 0 ? key & 0xFFFF : 0;
  return o;
}

// ssw_align's score1 and ref_begin1 for query q[0, qn) against the read ref[0, rn)
template <int R>
__device__ __forceinline__ void tr_align(const TrimArgs &a, const uint8_t *q, int qn, const uint8_t *ref, int rn, int lane, int &score,
                                         int &ref_begin) {
  const TrAln f = tr_sw_pass<R>(a, q, 1, qn, ref, 1, rn, -1, lane);
  score = f.score;
  ref_begin = -1;
  if (f.score > 0) {
    const TrAln b = tr_sw_pass<R>(a, q + f.end_row, -1, f.end_row + 1, ref + f.end_col, -1, f.end_col + 1, f.score, lane);
    ref_begin = b.end_col >= 0 ? f.end_col - b.end_col : -1;
  }
}

__global__ void __launch_bounds__(64) kc_trim_align_kernel(TrimArgs a, uint32_t nlist) {
  __shared__ uint32_t seen[TR_MAX_ENTRIES / 32];  // entries already aligned for this read (adapters_matching, :180)
  const int lane = threadIdx.x;
  const uint64_t end = a.offsets[a.nreads];
  const int nwords = (int)((a.n_entries + 31u) / 32u);
  unsigned long long st[TRS_N] = {0, 0, 0, 0};
  for (uint32_t li = blockIdx.x; li < nlist; li += gridDim.x) {
    const uint32_t rd = a.list[li];
    const uint64_t off = a.offsets[rd];
    const int len = (int)(a.offsets[rd + 1] - off);
    const uint8_t *ref = a.bases + off;
    for (int w = lane; w < nwords; w += 64) seen[w] = 0;
    mg_wave_sync();
    double best_identity = 0.0;
    int best_pos = len;
    bool found = false;
    for (int c0 = 0; TR_STEP * c0 + a.k <= len && !found; c0 += TR_CHUNK) {
      uint64_t key;
      uint32_t rs = 0, rc = 0;
      if (tr_seed_keys(a.bases, off, len, c0, lane, a.k, end, key)) rc = tr_lookup(a, key, rs);
      uint64_t m = __ballot(rc != 0);
      while (m && !found) {  // the k-mers in the index, in position order
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int i = TR_STEP * (c0 + l);
        const uint32_t s0 = __shfl(rs, l), cnt = __shfl(rc, l);
        for (uint32_t b = 0; b < cnt; b += 64) {  // the first record whose entry was not aligned yet
          uint32_t rec = 0;
          bool fresh = false;
          if (b + lane < cnt) {
            rec = a.recs[s0 + b + lane];
            const uint32_t e = rec >> TR_REC_OFF_BITS;
            fresh = !((seen[e >> 5] >> (e & 31u)) & 1u);
          }
          const uint64_t fm = __ballot(fresh);
          if (!fm) continue;
          rec = __shfl(rec, __ffsll((unsigned long long)fm) - 1);
          const uint32_t e = rec >> TR_REC_OFF_BITS;
          const int koff = (int)(rec & ((1u << TR_REC_OFF_BITS) - 1u));
          if (lane == 0) seen[e >> 5] |= 1u << (e & 31u);
          mg_wave_sync();
          const uint32_t eo = a.ent_off[e];
          const int alen = (int)(a.ent_off[e + 1] - eo);
          const int start = koff - i - 2 > 0 ? koff - i - 2 : 0;  // :201-203
          int qn = start + len + 2 < alen ? start + len + 2 : alen;
          if (qn > alen - start) qn = alen - start;
          int score, rb;
          if (qn <= 128)
            tr_align<2>(a, a.ent_bytes + eo + start, qn, ref, len, lane, score, rb);
          else
            tr_align<TR_MAX_ENTRY_LEN / 64>(a, a.ent_bytes + eo + start, qn, ref, len, lane, score, rb);
          st[TRS_ALIGN]++;
          const int mml = alen < len - rb ? alen : len - rb;  // :209
          const double identity = (double)score / (double)a.match / (double)mml;
          if (identity >= best_identity) {
            best_identity = identity;
            best_pos = rb;
            if (identity > 0.97) found = true;
          }
          break;  // :240
        }
      }
    }
    if (best_identity >= 0.5) {  // :247-256
      if (best_pos < TR_MIN_TRIM_POS) best_pos = 0;
      st[TRS_TRIMMED]++;
      st[TRS_BASES] += (unsigned long long)(len - best_pos);
      if (!best_pos) st[TRS_REMOVED]++;
      if (lane == 0) a.res[rd] = (uint32_t)best_pos | TR_RES_TRIMMED;
    }
    mg_wave_sync();
  }
  if (lane == 0)
    for (int f = 0; f < TRS_N; f++)
      if (st[f]) atomicAdd(&a.stats[f], st[f]);
}

// final lengths (trim_pair's rule, :265-271) and the bytes of every tile
__global__ void __launch_bounds__(TR_TILE) kc_trim_sizes_kernel(TrimArgs a) {
  __shared__ uint64_t wsum[TR_TILE / 64];
  const uint64_t r = (uint64_t)blockIdx.x * TR_TILE + threadIdx.x;
  uint32_t n = 0;
  if (r < a.nreads) {
    const uint32_t me = a.res[r];
    n = me & ~TR_RES_TRIMMED;
    if (a.paired) {
      const uint32_t ot = a.res[r ^ 1ull];
      const uint32_t on = ot & ~TR_RES_TRIMMED;
      if (((me | ot) & TR_RES_TRIMMED) && n > 1u && on > 1u) n = n < on ? n : on;
    }
    a.flen[r] = n;
  }
  uint64_t s = n;
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int w = 0; w < TR_TILE / 64; w++) t += wsum[w];
    a.tile_bytes[blockIdx.x] = t;
  }
}

// tile_bytes holds the exclusive scan: in-tile offsets, then the bytes
__global__ void __launch_bounds__(TR_TILE) kc_trim_write_kernel(TrimArgs a) {
  __shared__ uint64_t wsum[TR_TILE / 64];
  __shared__ uint64_t obase[TR_TILE];
  __shared__ uint32_t olen[TR_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t r0 = (uint64_t)blockIdx.x * TR_TILE;
  const uint64_t r = r0 + tid;
  const uint32_t n = r < a.nreads ? a.flen[r] : 0u;
  uint64_t inc = n;
  for (int s = 1; s < 64; s <<= 1) {
    const uint64_t v = __shfl_up(inc, s);
    if (lane >= s) inc += v;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint64_t base = a.tile_bytes[blockIdx.x];
  for (int w = 0; w < wv; w++) base += wsum[w];
  obase[tid] = base + inc - n;
  olen[tid] = n;
  if (r < a.nreads) a.out_offsets[r + 1] = base + inc;
  if (r == 0) a.out_offsets[0] = 0;
  __syncthreads();
  const int nr = a.nreads - r0 < (uint64_t)TR_TILE ? (int)(a.nreads - r0) : TR_TILE;
  for (int j = wv; j < nr; j += TR_TILE / 64) {  // a wave copies a read
    const uint64_t src = a.offsets[r0 + j], dst = obase[j];
    const int len = (int)olen[j];
    for (int t = lane; t < len; t += 64) {
      a.out_bases[dst + t] = a.bases[src + t];
      a.out_quals[dst + t] = a.quals[src + t];
    }
  }
}

}  // namespace kc
