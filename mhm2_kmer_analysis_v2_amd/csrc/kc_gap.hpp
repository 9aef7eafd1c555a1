// kc_gap.hpp -- gapped refinement of kc_align_reads' records (kc_align_gapped): the role of klign's SSW fallback.  The
// step around the dynamic programme is this project's own definition (pinned statement by
// statement by tests/gap_model.py); the dynamic programme is the reference's ssw_align (src/ssw/ssw_core.cpp:200-403,
// 874-955) as kc_trim.hpp states it and tests/trim_model.py::ssw_align restates it, here with all five results: score,
// the reference interval and the query interval (tests/golden/gap_ref_alignments.json pins them on read-sized inputs).
//
// Rules:
//  * A record (kc_read_aln) is valid iff read < nreads, ctg < n_ctgs, orient <= 1, cstart < cstop <= len_u,
//    rstart < rstop <= L, cstop - cstart == rstop - rstart and, with d = cstart - rstart, cstart == max(0, d) and
//    cstop == min(len_u, d + L).  The input's mismatches field is not read.
//  * Codes: a read's A C G T in either case are 0..3, anything else 4 (kc_align_reads' alphabet: U is 4); a contig's
//    A C G T are 0..3, N is 4.  R' is the read (orient 0) or its reverse complement (code c < 4 -> 3 - c).
//  * mismatches = the i in [rstart, rstop) where R'[i] is 4, contig[d + i] is 4, or the two differ.
//  * mismatches == 0 without KC_GAP_ALWAYS_DP: the input interval, score = match * (rstop - rstart), KC_GAP_EXACT.
//  * Otherwise ssw_align of all of R' (L rows) against contig[wlo, whi), wlo = max(0, d - pad),
//    whi = min(len_u, d + L + pad).  score > 0: cstart = wlo + ref_begin, cstop = wlo + ref_end + 1,
//    rstart = query_begin, rstop = query_end + 1 (KC_GAP_DP); score 0: four zeros (KC_GAP_NONE).
//
// Kernels:
//  kc_gap_check_kernel   a thread per record: validity, the lowest bad index by a 64-bit atomicMin.  Writes no record.
//  kc_gap_sort_kernel    a wave per record: the recount (64 positions a trip, coalesced on both sides), then either the
//                        exact record or an entry index | mismatches << 32 in a list.  A record's slot in the output is
//                        its index, so the order of the list does not matter.
//  kc_gap_dp_kernel<R>   a wave per listed record, R rows a lane (R' as codes in registers, loaded once per pass).  A
//                        column lies across the lanes; the window's codes come 64 columns at a time, coalesced, and are
//                        broadcast.  The F dependency down a column is a prefix maximum over the wave, as in
//                        kc_trim.hpp's tr_sw_pass; the second pass (reversed prefix of R' against the window from
//                        ref_end downwards, until a column holds the score) runs in the same wave.  Trip counts are
//                        wave-uniform and bounded by L and the window's length; no wave waits for another.
#pragma once
#include "kc_align.hpp"

namespace kc {

constexpr int GAP_TPB = 256;
constexpr int GAP_WAVES = GAP_TPB / 64;
constexpr uint32_t GAP_MAX_PAD = 1024;  // KC_GAP_MAX_PAD
constexpr uint32_t GAP_ALWAYS_DP = 1;   // KC_GAP_ALWAYS_DP
constexpr uint32_t GAP_KIND_EXACT = 0, GAP_KIND_DP = 1, GAP_KIND_NONE = 2;
constexpr int GAP_NEG = -(1 << 28);

enum { GPS_BAD = 0, GPS_NLIST, GPS_EXACT, GPS_DP, GPS_NONE, GPS_CELLS, GPS_SCORE_SUM, GPS_COUNT };

struct GapArgs {
  AlignIndex ix;
  const uint8_t *bases;
  const uint64_t *offsets;
  uint64_t nreads;
  const uint4 *alns;  // kc_read_aln, two words of 16 bytes each
  uint64_t n_alns;
  uint4 *out;  // kc_gap_aln, the same
  uint32_t pad, flags;
  int match, mismatch, gap_open, gap_ext, amb;
  uint64_t *list;  // [n_alns] record index | mismatches << 32
  uint64_t *st;    // [GPS_COUNT]
};

// a record as the kernels use it
struct GapRec {
  uint32_t read, ctg, cstart, cstop, rstart, rstop, seeds, orient;
};

__device__ __forceinline__ GapRec gap_load(const uint4 *alns, uint64_t i) {
  const uint4 a = alns[2 * i], z = alns[2 * i + 1];
  GapRec r;
  r.read = a.x;
  r.ctg = a.y;
  r.cstart = a.z;
  r.cstop = a.w;
  r.rstart = z.x & 0xFFFFu;
  r.rstop = z.x >> 16;
  r.seeds = z.y >> 16;
  r.orient = z.z & 0xFFu;
  return r;
}

__device__ __forceinline__ void gap_store(uint4 *out, uint64_t i, const GapRec &r, uint32_t cstart, uint32_t cstop, uint32_t rstart,
                                          uint32_t rstop, uint32_t score, uint32_t mism, uint32_t kind) {
  uint4 a, z;
  a.x = r.read;
  a.y = r.ctg;
  a.z = cstart;
  a.w = cstop;
  z.x = rstart | (rstop << 16);
  z.y = score;
  z.z = mism | (r.seeds << 16);
  z.w = r.orient | (kind << 8);
  out[2 * i] = a;
  out[2 * i + 1] = z;
}

// a read's byte as a code: A C G T in either case, else 4
__device__ __forceinline__ int gap_read_code(uint32_t c) { return kc_is_acgt(c) ? (int)kc_base_code(c) : 4; }
// a contig's byte (A C G T N by the index's own check)
__device__ __forceinline__ int gap_ctg_code(uint32_t c) { return c == 'N' ? 4 : (int)kc_base_code(c); }
// R'[i] of a read of L bases at rd
__device__ __forceinline__ int gap_rprime(const uint8_t *rd, uint32_t L, uint32_t orient, uint32_t i) {
  const int c = gap_read_code(rd[orient ? L - 1u - i : i]);
  return (orient && c < 4) ? 3 - c : c;
}

__global__ void kc_gap_check_kernel(GapArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_alns) return;
  const GapRec r = gap_load(a.alns, i);
  bool ok = (uint64_t)r.read < a.nreads && r.ctg < a.ix.n_ctgs && r.orient <= 1u;
  if (ok) {
    const int64_t L = (int64_t)(a.offsets[r.read + 1] - a.offsets[r.read]);  // <= ALIGN_MAX_READ_LEN (kc_align_lengths_kernel)
    const int64_t len = (int64_t)(a.ix.offs[r.ctg + 1] - 1u - a.ix.offs[r.ctg]);
    const int64_t cs = r.cstart, ce = r.cstop, rs = r.rstart, re = r.rstop;
    const int64_t d = cs - rs;
    ok = cs < ce && ce <= len && rs < re && re <= L && ce - cs == re - rs;
    ok = ok && cs == (d > 0 ? d : 0) && ce == (d + L < len ? d + L : len);
  }
  if (!ok) atomicMin((unsigned long long *)&a.st[GPS_BAD], (unsigned long long)i);
}

// A wave per record (every record is valid: kc_gap_check_kernel ran).
__global__ void __launch_bounds__(GAP_TPB) kc_gap_sort_kernel(GapArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * GAP_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * GAP_WAVES;
  unsigned long long n_exact = 0, score_sum = 0;
  for (uint64_t i = wave; i < a.n_alns; i += nwaves) {
    const GapRec r = gap_load(a.alns, i);
    const uint64_t r0 = a.offsets[r.read];
    const uint32_t L = (uint32_t)(a.offsets[r.read + 1] - r0);
    const uint8_t *rd = a.bases + r0;
    // block position that pairs with R'[0]; only [rstart, rstop) is read
    const int64_t cbase = (int64_t)a.ix.offs[r.ctg] + (int64_t)r.cstart - (int64_t)r.rstart;
    uint32_t mism = 0;
    for (uint32_t b = r.rstart; b < r.rstop; b += 64u) {
      const uint32_t p = b + (uint32_t)lane;
      bool bad = false;
      if (p < r.rstop) {
        const int q = gap_rprime(rd, L, r.orient, p);
        const int c = gap_ctg_code(a.ix.seqs[cbase + (int64_t)p]);
        bad = q == 4 || c == 4 || q != c;
      }
      mism += wave_count(bad);
    }
    if (mism == 0 && !(a.flags & GAP_ALWAYS_DP)) {
      const uint32_t score = (uint32_t)a.match * (r.rstop - r.rstart);
      if (lane == 0) gap_store(a.out, i, r, r.cstart, r.cstop, r.rstart, r.rstop, score, 0u, GAP_KIND_EXACT);
      n_exact++;
      score_sum += score;
    } else if (lane == 0) {
      const unsigned long long at = atomicAdd((unsigned long long *)&a.st[GPS_NLIST], 1ull);
      a.list[at] = i | ((uint64_t)mism << 32);
    }
  }
  if (lane == 0 && n_exact) {
    atomicAdd((unsigned long long *)&a.st[GPS_EXACT], n_exact);
    atomicAdd((unsigned long long *)&a.st[GPS_SCORE_SUM], score_sum);
  }
}

struct GapEnd {
  int score, end_col, end_row;
};

// One pass of the aligner.  Query row j, j < qn, is R'[q0 + j * qstep] (lane l holds rows l * R .. l * R + R - 1); column
// c, c < rn, is the block byte ref[c * rstep], in scan order.  term: stop at the first column whose maximum is that score
// (0: never).  Wave-uniform result: the best score, its first column (-1: score 0) and the smallest row holding it there.
//
// A column in two sweeps over the lane's rows.  First the uncorrected H (hp = max(diag + s, E, 0)) and what the lane's own
// rows hand on as F to the row below its last (o: F(t + 1) = max(F(t) - ext, hp(t) - open), started from nothing).  A lane
// l' contributes o(l') - (l - 1 - l') R ext to the F entering lane l, so a prefix maximum over o(l') + l' R ext gives every
// lane its F; the second sweep runs the same recurrence from there and corrects H.  E takes the uncorrected H
// (ssw_core.cpp:295).
// The substitution score is looked up, not selected: the column's five scores + 9 sit in one uniform word, five bits
// each, and a row holds its shift.  A row at or behind qn holds code 4 and is otherwise computed like any other: its H
// never exceeds a real row's of the same or an earlier column (it is reached by a diagonal step scoring -ambiguity <= 0
// from the column before, or by a gap, which costs), and equals it only in a later column, so it never wins the ending
// cell and never ends the second pass early.  The best cell is a maximum over h << 16 | (0xFFFF - (column << 4 | t)).
template <int R>
__device__ __forceinline__ GapEnd gap_sw_pass(const GapArgs &a, const uint8_t *rd, uint32_t L, uint32_t orient, int q0, int qstep, int qn,
                                              const uint8_t *ref, int rstep, int rn, int term, int lane) {
  constexpr int QW = (R + 3) / 4;
  int H[R], E[R];
  uint32_t qs[QW];  // 5 * the row's code, a byte each
#pragma unroll
  for (int w = 0; w < QW; w++) qs[w] = 0;
#pragma unroll
  for (int t = 0; t < R; t++) {
    const int row = lane * R + t;
    const int code = row < qn ? gap_rprime(rd, L, orient, (uint32_t)(q0 + row * qstep)) : 4;
    qs[t >> 2] |= (uint32_t)(5 * code) << (8 * (t & 3));
    H[t] = E[t] = 0;
  }
#pragma unroll
  for (int w = 0; w < QW; w++) asm volatile("" : "+v"(qs[w]));  // one register a word, not one a byte
  uint32_t W[5];  // W[r]: the scores of a column of code r against the codes 0..4
#pragma unroll
  for (int r = 0; r < 5; r++) {
    W[r] = 0;
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const int s = (r == 4 || q == 4) ? -a.amb : (r == q ? a.match : -a.mismatch);
      W[r] |= (uint32_t)(s + 9) << (5 * q);
    }
  }
  const int go = a.gap_open, ge = a.gap_ext;
  const int lane_w = lane * R * ge;  // what R rows of extension cost, times the lanes above
  uint32_t lbp = 0;
  bool done = false;
#pragma unroll 1
  for (int c0 = 0; c0 < rn && !done; c0 += 64) {
    const int ci = c0 + lane;
    const int cr = ci < rn ? gap_ctg_code(ref[(long)ci * rstep]) : 4;
    const uint32_t wl = cr == 0 ? W[0] : cr == 1 ? W[1] : cr == 2 ? W[2] : cr == 3 ? W[3] : W[4];
    const int cnt = rn - c0 < 64 ? rn - c0 : 64;
#pragma unroll 1
    for (int c = 0; c < cnt; c++) {
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)wl, c);
      int prev = __shfl_up(H[R - 1], 1);
      if (lane == 0) prev = 0;
      int e2[R];  // the uncorrected H less the gap open penalty: what E and F take from it
      int o = GAP_NEG;
#pragma unroll
      for (int t = 0; t < R; t++) {
        const uint32_t sh = (qs[t >> 2] >> (8 * (t & 3))) & 0xFFu;
        const int s = (int)((w >> sh) & 31u);
        const int d = prev + s - 9;
        prev = H[t];
        int h = d > E[t] ? d : E[t];
        h = h > 0 ? h : 0;
        e2[t] = h - go;
        const int o1 = o - ge;
        o = o1 > e2[t] ? o1 : e2[t];
      }
      int inc = o + lane_w;  // inclusive prefix maximum over the lanes
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const int v = __shfl_up(inc, s);
        if (lane >= s) inc = inc > v ? inc : v;
      }
      int f = __shfl_up(inc, 1) - (lane_w - R * ge);  // the F entering this lane's first row
      if (lane == 0) f = GAP_NEG;
      const uint32_t kc = 0xFFFFu - ((uint32_t)(c0 + c) << 4);
      int cmx = 0;
#pragma unroll
      for (int t = 0; t < R; t++) {
        const int fo = f - go;
        const int h = (e2[t] > fo ? e2[t] : fo) + go;
        H[t] = h;
        const int e1 = E[t] - ge, f1 = f - ge;
        E[t] = e1 > e2[t] ? e1 : e2[t];  // ssw_core.cpp:295: from H before F's correction
        f = f1 > e2[t] ? f1 : e2[t];
        cmx = cmx > h ? cmx : h;
        const uint32_t pk = ((uint32_t)h << 16) + (kc - (uint32_t)t);
        lbp = lbp > pk ? lbp : pk;
      }
      if (term > 0 && __ballot(cmx == term) && !__ballot(cmx > term)) {  // the column's maximum is the score
        done = true;
        break;
      }
    }
  }
  const int lbest = (int)(lbp >> 16);
  int best = lbest;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int v = __shfl_xor(best, s);
    best = best > v ? best : v;
  }
  const uint32_t lk = 0xFFFFu - (lbp & 0xFFFFu);  // column << 4 | t
  int key = (lbest == best && best > 0) ? (int)(((lk >> 4) << 16) | ((uint32_t)(lane * R) + (lk & 15u))) : 0x7FFFFFFF;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int v = __shfl_xor(key, s);
    key = key < v ? key : v;
  }
  GapEnd o;
  o.score = best;
  o.end_col = best > 0 ? key >> 16 : -1;
  o.end_row = best > 0 ? key & 0xFFFF : 0;
  return o;
}

// A wave per listed record; R * 64 >= the longest read of the call.
template <int R>
__global__ void __launch_bounds__(GAP_TPB) __attribute__((amdgpu_waves_per_eu(4))) kc_gap_dp_kernel(GapArgs a, uint64_t nlist) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * GAP_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * GAP_WAVES;
  unsigned long long n_dp = 0, n_none = 0, cells = 0, score_sum = 0;
  for (uint64_t li = wave; li < nlist; li += nwaves) {
    const uint64_t e = a.list[li];
    const uint64_t i = e & 0xFFFFFFFFull;
    const uint32_t mism = (uint32_t)(e >> 32);
    const GapRec r = gap_load(a.alns, i);
    const uint64_t r0 = a.offsets[r.read];
    const uint32_t L = (uint32_t)(a.offsets[r.read + 1] - r0);
    const uint8_t *rd = a.bases + r0;
    const uint32_t c0 = a.ix.offs[r.ctg];
    const int64_t len = (int64_t)(a.ix.offs[r.ctg + 1] - 1u - c0);
    const int64_t d = (int64_t)r.cstart - (int64_t)r.rstart;
    const int64_t lo = d - (int64_t)a.pad, hi = d + (int64_t)L + (int64_t)a.pad;
    const int64_t wlo = lo > 0 ? lo : 0, whi = hi < len ? hi : len;  // wlo <= cstart < cstop <= whi
    const uint8_t *win = a.ix.seqs + c0 + wlo;
    const int wn = (int)(whi - wlo);
    cells += (unsigned long long)L * (unsigned long long)wn;
    const GapEnd f = gap_sw_pass<R>(a, rd, L, r.orient, 0, 1, (int)L, win, 1, wn, 0, lane);
    if (f.score > 0) {
      const GapEnd b = gap_sw_pass<R>(a, rd, L, r.orient, f.end_row, -1, f.end_row + 1, win + f.end_col, -1, f.end_col + 1, f.score, lane);
      const uint32_t ref_begin = (uint32_t)(f.end_col - b.end_col), query_begin = (uint32_t)(f.end_row - b.end_row);
      if (lane == 0)
        gap_store(a.out, i, r, (uint32_t)wlo + ref_begin, (uint32_t)wlo + (uint32_t)f.end_col + 1u, query_begin, (uint32_t)f.end_row + 1u,
                  (uint32_t)f.score, mism, GAP_KIND_DP);
      n_dp++;
      score_sum += (unsigned long long)f.score;
    } else {
      if (lane == 0) gap_store(a.out, i, r, 0u, 0u, 0u, 0u, 0u, mism, GAP_KIND_NONE);
      n_none++;
    }
  }
  if (lane == 0) {
    if (n_dp) atomicAdd((unsigned long long *)&a.st[GPS_DP], n_dp);
    if (n_none) atomicAdd((unsigned long long *)&a.st[GPS_NONE], n_none);
    if (cells) atomicAdd((unsigned long long *)&a.st[GPS_CELLS], cells);
    if (score_sum) atomicAdd((unsigned long long *)&a.st[GPS_SCORE_SUM], score_sum);
  }
}

}  // namespace kc
