// kc_close.hpp -- closing scaffold gaps from splint reads (kc_close_gaps): a read aligned across two contigs carries the
// bases between their ends; where enough reads agree on the distance, the N run of a join becomes their consensus, an
// abutment or a verified overlap -- the step behind kc_scaffold.hpp.  The reference holds no code for it (src/contigging.cpp
// stops before scaffolding), so the rules are this project's own definition (pinned statement by
// statement by tests/close_model.py); no parity with MetaHipMer is claimed.  include/kcount_mi355.h states the rules in full.
//
// Nodes and ends are kc_scaffold.hpp's: node v = 2u + s is entered through end v and left through end v ^ 1.  Member m (not
// a head) follows member m - 1: the join is left through ea = node(m - 1) ^ 1 and entered through fb = node(m).  Every
// contig is a member once, so every end belongs to at most one join.
//
// Kernels, in the order of the call (in front of them kc_align_lengths_kernel and kc_depth_check_kernel check the reads and
// the records; kc_link_group_kernel<false / true>, kc_link_tile_scan_kernel and kc_scan_kernel<1> group the passing records
// by read, all as they stand):
//  kc_close_check_scaf_kernel    a thread per scaffold record: its own rules and its predecessor's end; marks the heads.
//  kc_close_claim_kernel         a thread per member: the lowest member index of every contig (32-bit atomic minimum).
//  kc_close_check_member_kernel  a thread per member: its rules; the lowest bad index by a 64-bit atomic minimum.
//  kc_close_ends_kernel          a thread per member: a gap join files itself under its two ends (end -> join << 1 | side).
//  kc_close_cands_kernel<W>      a thread per read, run twice: every ordered pair of the read's slots, as
//                                kc_link_cands_kernel forms them, looked up in the end table.  W = false counts a join's
//                                candidates (one 64-bit atomic each) and the statistics; the two-level scan makes the counts
//                                the joins' first slots; W = true takes a slot through the join's cursor and writes {where
//                                the segment starts in the reads' bytes, gap, direction} as one 16-byte store.  The order
//                                inside a join is left free: every later figure is a count or a vote.
//  kc_close_decide_kernel        a WAVE per member.  A gap join's lanes stride over its candidates, each counting the
//                                candidates of its own gap value (k * k / 64 trips for k candidates: a join has as many as
//                                the reads' depth, no sort is worth its launches), six butterfly steps keep (most votes,
//                                smallest gap); an overlap is compared with the contigs' text 64 bytes a trip.  Writes the
//                                member's decision, its segment's bytes and its fill's bytes, and counts nothing.
//  kc_close_place_kernel         a thread per member behind the two scans: the segment's start in the block, the fill's in
//                                the fill buffer, the member and closure records, the scaffold's N and overlap bases
//                                (32-bit integer atomics; the scaffold by binary search over the first members), and the
//                                call's statistics, one atomic a workgroup of 1024 members and counter.
//  kc_close_vote_kernel          a wave per member, at work for a filled join: lanes are columns, 64 consecutive read bytes
//                                a trip and supporter (backward supporters from the segment's far end, complemented), four
//                                32-bit counters a lane; the winner goes to the fill buffer, a byte a lane.  Sixteen joins a
//                                workgroup, one atomic a workgroup for the disputed columns.
//  kc_close_records_kernel       a thread per scaffold: its 32-byte record and its offset.
//  kc_close_write_kernel         a thread per ALIGNED 16 bytes of the block, as kc_scaf_write_kernel: binary search over the
//                                segments' starts, then on over as many members as its bytes span -- N run or fill, text
//                                forwards or reverse-complemented, separators -- and one 16-byte store; the block's first and
//                                last partial chunk are byte stores.  The only kernel that stores to the block.
//
// Plain vector stores only; no workgroup waits for another; every loop's trip count comes from the input (a read's slots,
// a join's candidates, a fill's columns, an overlap's length, a search's steps, the members a chunk spans).  All figures
// are integers, so the result does not depend on the order in which the atomics arrive.
#pragma once
#include "kc_scaffold.hpp"

namespace kc {

constexpr int CLOSE_TPB = 256;
constexpr uint32_t CLOSE_NONE = 0xFFFFFFFFu;
enum { CLOSE_HEAD = 0, CLOSE_NOT_A_GAP, CLOSE_NO_READS, CLOSE_WEAK, CLOSE_FILLED, CLOSE_ABUT, CLOSE_OVERLAP, CLOSE_OVERLAP_REJECTED };

// device statistics of a call (uint64_t each)
enum { CLS_BAD = 0, CLS_OVER_CAP, CLS_CANDS, CLS_OFF_JOIN, CLS_GAPS, CLS_NO_READS, CLS_WEAK, CLS_FILLED, CLS_ABUT, CLS_OVERLAP, CLS_OV_REJECTED,
       CLS_FILL_BASES, CLS_N_LEFT, CLS_DISPUTED, CLS_JCAND_TOTAL, CLS_SEG_TOTAL, CLS_FILL_TOTAL, CLS_COUNT };

struct CloseArgs {
  const uint64_t *offsets;  // the reads'
  uint64_t nreads;
  const uint64_t *rfirst, *rbase;  // the reads' first slots: within their tile, and the tiles'
  const uint32_t *rcur;            // the reads' passing records
  const uint4 *info;               // the slots, as kc_link_group_kernel<true> writes them
  const uint32_t *table;           // [2 n_ctgs] end -> join << 1 | (the end is the join's fb), or CLOSE_NONE
  uint32_t max_overlap, max_splint_gap, max_read_alns;
  uint64_t *jcnt;         // [members] a join's candidates, then its first slot within its tile
  const uint64_t *jbase;  // [tiles of members]
  uint32_t *jcur;         // [members] cursors of the write pass: the joins' candidates when it is done
  uint4 *cands;           // [candidates on a join] {segment start lo, hi, gap, backward}
  uint64_t *st;
};

__device__ __forceinline__ uint32_t close_len(const uint32_t *offs, uint32_t u) { return offs[u + 1] - 1u - offs[u]; }

// scaf: kc_scaffold_rec as two uint4 {first_member, n_members, len, n_bases} {overlap_bases, flags, 0, 0}; ishead: zeroed
__global__ void __launch_bounds__(CLOSE_TPB) kc_close_check_scaf_kernel(const uint4 *scaf, uint64_t n_scaf, uint32_t n, uint32_t *ishead,
                                                                        uint64_t *st) {
  const uint64_t s = (uint64_t)blockIdx.x * CLOSE_TPB + threadIdx.x;
  if (s >= n_scaf) return;
  const uint4 a = scaf[2 * s];
  uint64_t want = 0;
  if (s) {
    const uint4 p = scaf[2 * (s - 1)];
    want = (uint64_t)p.x + p.y;
  }
  const uint64_t end = (uint64_t)a.x + a.y;
  const bool ok = a.y >= 1u && a.x == want && end <= n && (s + 1 < n_scaf || end == n);
  if (ok)
    ishead[a.x] = 1u;  // a.x < end <= n
  else
    atomicMin((unsigned long long *)&st[CLS_BAD], (unsigned long long)s);
}

// members: kc_scaf_member as a uint4 {ctg, join, out_pos, orient | pad << 8}; owner: 0xFF-filled
__global__ void __launch_bounds__(CLOSE_TPB) kc_close_claim_kernel(const uint4 *members, uint32_t n, uint32_t *owner) {
  const uint64_t m = (uint64_t)blockIdx.x * CLOSE_TPB + threadIdx.x;
  if (m >= n) return;
  const uint32_t u = members[m].x;
  if (u < n) atomicMin(&owner[u], (uint32_t)m);
}

__global__ void __launch_bounds__(CLOSE_TPB) kc_close_check_member_kernel(const uint4 *members, uint32_t n, const uint32_t *ishead,
                                                                          const uint32_t *owner, const uint32_t *offs, uint64_t *st) {
  const uint64_t m = (uint64_t)blockIdx.x * CLOSE_TPB + threadIdx.x;
  if (m >= n) return;
  const uint4 a = members[m];
  const int32_t j = (int32_t)a.y;
  bool ok = a.x < n && a.w <= 1u;  // orient <= 1 and the three reserved bytes zero
  ok = ok && owner[a.x] == (uint32_t)m;
  if (ok) {
    if (ishead[m])
      ok = j == 0;
    else {
      ok = j >= -(int32_t)LINK_MAX_OVERLAP && j <= (int32_t)PAIR_INSERT_MAX;
      if (ok && j < 0) {
        const uint32_t pu = members[m - 1].x;  // m >= 1: member 0 is a head; a bad predecessor is the lower index anyway
        if (pu < n) {
          const uint32_t la = close_len(offs, pu), lb = close_len(offs, a.x);
          ok = (uint32_t)-j < (la < lb ? la : lb);
        }
      }
    }
  }
  if (!ok) atomicMin((unsigned long long *)&st[CLS_BAD], (unsigned long long)m);
}

// table: 0xFF-filled, 2 n entries
__global__ void __launch_bounds__(CLOSE_TPB) kc_close_ends_kernel(const uint4 *members, uint32_t n, const uint32_t *ishead, uint32_t *table) {
  const uint64_t m = (uint64_t)blockIdx.x * CLOSE_TPB + threadIdx.x;
  if (m >= n || ishead[m]) return;
  const uint4 b = members[m];
  if ((int32_t)b.y <= 0) return;
  const uint4 a = members[m - 1];
  table[(2u * a.x + a.w) ^ 1u] = (uint32_t)m << 1;
  table[2u * b.x + b.w] = ((uint32_t)m << 1) | 1u;
}

template <bool WRITE>
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_close_cands_kernel(CloseArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t on = 0, off = 0, over = 0;
  if (t < a.nreads) {
    const uint64_t f = a.rbase[t >> LINK_SCAN_SHIFT] + a.rfirst[t], c = a.rcur[t];
    if (c > (uint64_t)a.max_read_alns)
      over = 1;
    else {
      const uint64_t r0 = a.offsets[t];
      for (uint64_t i = 0; i < c; i++) {
        const uint4 x = a.info[f + i];
        if (x.z == LINK_NO_END) continue;  // it does not leave
        const int64_t qs_a = x.x & 0xFFFFu, qe_a = x.x >> 16;
        for (uint64_t j = 0; j < c; j++) {
          const uint4 y = a.info[f + j];
          const int64_t qs_b = y.x & 0xFFFFu, qe_b = y.x >> 16;
          if ((x.y >> 1) == (y.y >> 1) || y.w == LINK_NO_END || !(qs_a < qs_b && qe_a < qe_b)) continue;
          const int64_t gap = (qs_b - qe_a) - (int64_t)x.z - (int64_t)y.w;
          if (gap < -(int64_t)a.max_overlap || gap > (int64_t)a.max_splint_gap) continue;
          // X = x.y ^ 1 is the end a leaves through, Y = y.y the end b enters through; two different ends of one join are
          // its ea and fb: forward iff X is the ea
          const uint32_t jx = a.table[x.y ^ 1u], jy = a.table[y.y];
          if (jx == CLOSE_NONE || (jx >> 1) != (jy >> 1)) {
            off++;
            continue;
          }
          on++;
          const uint32_t m = jx >> 1;
          if (!WRITE)
            atomicAdd((unsigned long long *)&a.jcnt[m], 1ull);
          else {
            const uint64_t slot = a.jbase[m >> LINK_SCAN_SHIFT] + a.jcnt[m] + (uint64_t)atomicAdd(&a.jcur[m], 1u);
            const uint64_t seg = r0 + (uint64_t)(qe_a + (int64_t)x.z);
            a.cands[slot] = make_uint4((uint32_t)seg, (uint32_t)(seg >> 32), (uint32_t)(int32_t)gap, jx & 1u);
          }
        }
      }
    }
  }
  if (!WRITE) {
    const int k[3] = {CLS_CANDS, CLS_OFF_JOIN, CLS_OVER_CAP};
    const uint32_t mine[3] = {on + off, off, over};
    wg_stats<3>(a.st, k, mine);
  }
}

// dec[m] = {new join, status, the chosen gap's candidates, the join's candidates}; seglen[m]: the bytes of the member's
// segment (run or fill, text, the separator behind a scaffold's last member); filllen[m]: the fill's bytes
__global__ void __launch_bounds__(CLOSE_TPB) kc_close_decide_kernel(const uint4 *members, uint32_t n, const uint32_t *ishead, const uint64_t *jfirst,
                                                                    const uint64_t *jbase, const uint32_t *jcur, const uint4 *cands,
                                                                    uint32_t min_reads, uint32_t permille, const uint8_t *seqs, const uint32_t *offs,
                                                                    uint4 *dec, uint64_t *seglen, uint64_t *filllen) {
  const int lane = threadIdx.x & 63;
  const uint64_t m = (uint64_t)blockIdx.x * (CLOSE_TPB / 64) + (threadIdx.x >> 6);
  if (m >= n) return;  // the whole wave
  const uint4 b = members[m];
  const bool head = ishead[m] != 0u;
  const int32_t old = (int32_t)b.y;
  const uint32_t lb = close_len(offs, b.x);
  int32_t join = old;
  uint32_t status = head ? CLOSE_HEAD : CLOSE_NOT_A_GAP, votes = 0, k = 0;
  if (!head && old > 0) {
    k = jcur[m];
    const uint64_t f = jbase[m >> LINK_SCAN_SHIFT] + jfirst[m];
    // (votes, smaller gap) as one word: votes << 32 | ~(gap + 2^31)
    uint64_t best = 0;
    for (uint32_t i = lane; i < k; i += 64) {
      const uint32_t g = cands[f + i].z;
      uint32_t v = 0;
      for (uint32_t q = 0; q < k; q++) v += cands[f + q].z == g ? 1u : 0u;
      const uint64_t w = ((uint64_t)v << 32) | (uint32_t)~(g + 0x80000000u);
      best = w > best ? w : best;
    }
    best = wave_max(best);
    status = CLOSE_NO_READS;
    if (k) {
      const uint32_t v = (uint32_t)(best >> 32);
      const int32_t g = (int32_t)(~(uint32_t)best - 0x80000000u);
      status = CLOSE_WEAK;
      if (v >= min_reads && (uint64_t)v * 1000ull >= (uint64_t)k * permille) {
        votes = v;
        if (g > 0) {
          status = CLOSE_FILLED;
          join = g;
        } else if (g == 0) {
          status = CLOSE_ABUT;
          join = 0;
        } else {
          // A: the node before, its last o bytes; B: this node, its first o bytes
          const uint4 pa = members[m - 1];
          const uint32_t la = close_len(offs, pa.x), o = (uint32_t)-g;
          const uint8_t *sa = seqs + offs[pa.x], *sb = seqs + offs[b.x];
          const bool ra = pa.w != 0u, rb = b.w != 0u;
          bool same = o < (la < lb ? la : lb);
          for (uint32_t i0 = 0; i0 < o && same; i0 += 64) {
            const uint32_t i = i0 + lane;
            bool ok = true;
            if (i < o) {
              const uint32_t cb = scaf_text(sb, lb, rb, i);
              ok = ai_is_acgt_upper(cb) && scaf_text(sa, la, ra, la - o + i) == cb;
            }
            same = __ballot(!ok) == 0ull;
          }
          status = same ? CLOSE_OVERLAP : CLOSE_OVERLAP_REJECTED;
          if (same) join = g;
        }
      }
    }
  }
  if (lane) return;
  const uint32_t nrun = join > 0 ? (uint32_t)join : 0u, skip = join < 0 ? (uint32_t)-join : 0u;
  const bool last = m + 1 == n || ishead[m + 1] != 0u;
  dec[m] = make_uint4((uint32_t)join, status, votes, k);
  seglen[m] = (uint64_t)nrun + lb - skip + (last ? 1u : 0u);
  filllen[m] = status == CLOSE_FILLED ? nrun : 0u;
}

// segoff, filloff: seglen and filllen behind their tile scans, with the tiles' bases.  seg[i]: where member i's segment starts
// in the block, seg[n] = total; fill[i]: where its fill starts in the fill buffer, CLOSE_NONE without one.  members_out,
// closures (kc_closure as two uint4: {cands, reads, old_join, new_join} {fill_pos, disputed, status, 0}), acc (zeroed, {N
// bases, overlap bases} a scaffold; scaf_in: the scaffolds' first members, every other uint4) may be null.
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_close_place_kernel(const uint4 *members, uint32_t n, const uint4 *dec, const uint64_t *segoff,
                                                                       const uint64_t *segbase, const uint64_t *filloff, const uint64_t *fillbase,
                                                                       uint32_t total, const uint4 *scaf_in, uint64_t n_scaf, uint32_t *seg,
                                                                       uint32_t *fill, uint4 *members_w, uint4 *members_out, uint4 *closures,
                                                                       uint32_t *acc, uint64_t *st) {
  const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t status = CLOSE_HEAD, filled_bases = 0, n_left = 0;
  if (m < n) {
    if (m == 0) seg[n] = total;
    const uint4 a = members[m], d = dec[m];
    const int32_t join = (int32_t)d.x;
    const uint32_t at = (uint32_t)(segbase[m >> LINK_SCAN_SHIFT] + segoff[m]);
    const uint32_t nrun = join > 0 ? (uint32_t)join : 0u, skip = join < 0 ? (uint32_t)-join : 0u;
    const bool filled = d.y == CLOSE_FILLED;
    status = d.y;
    filled_bases = filled ? nrun : 0u;
    n_left = filled ? 0u : nrun;
    seg[m] = at;
    fill[m] = filled ? (uint32_t)(fillbase[m >> LINK_SCAN_SHIFT] + filloff[m]) : CLOSE_NONE;
    const uint4 rec = make_uint4(a.x, d.x, at + nrun, a.w);
    members_w[m] = rec;
    if (members_out) members_out[m] = rec;
    if (closures) {
      closures[2 * m] = make_uint4(d.w, d.z, a.y, d.x);
      closures[2 * m + 1] = make_uint4(at, 0u, d.y, 0u);
    }
    if (acc && (n_left || skip)) {
      // the scaffold that holds m: the first one's first member is 0
      const uint64_t s = find_le((uint64_t)0, n_scaf - 1, (uint32_t)m, [scaf_in](uint64_t mid) { return scaf_in[2 * mid].x; });
      if (n_left) atomicAdd(&acc[2 * s], n_left);
      if (skip) atomicAdd(&acc[2 * s + 1], skip);
    }
  }
  // the call's statistics: one atomic a workgroup and counter (a wave of every gap join adding to one address took half
  // the call's kernel time when the decide kernel counted them); a workgroup's sums fit 32 bits, a run has at most 65535 bytes
  const int k[9] = {CLS_GAPS, CLS_NO_READS, CLS_WEAK, CLS_FILLED, CLS_ABUT, CLS_OVERLAP, CLS_OV_REJECTED, CLS_FILL_BASES, CLS_N_LEFT};
  const uint32_t mine[9] = {status >= CLOSE_NO_READS ? 1u : 0u, status == CLOSE_NO_READS ? 1u : 0u, status == CLOSE_WEAK ? 1u : 0u,
                            status == CLOSE_FILLED ? 1u : 0u, status == CLOSE_ABUT ? 1u : 0u, status == CLOSE_OVERLAP ? 1u : 0u,
                            status == CLOSE_OVERLAP_REJECTED ? 1u : 0u, filled_bases, n_left};
  wg_stats<9>(st, k, mine);
}

// members_w, fill: as the place kernel wrote them; buf: the fill buffer; closures: may be null
__global__ void __launch_bounds__(LINK_STAT_TPB) kc_close_vote_kernel(const uint4 *dec, uint32_t n, const uint64_t *jfirst, const uint64_t *jbase,
                                                                      const uint32_t *jcur, const uint4 *cands, const uint8_t *bases,
                                                                      const uint32_t *fill, uint8_t *buf, uint4 *closures, uint64_t *st) {
  const int lane = threadIdx.x & 63;
  const uint64_t m = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  uint32_t disputed = 0;
  const uint4 d = m < n ? dec[m] : make_uint4(0u, CLOSE_HEAD, 0u, 0u);
  if (d.y == CLOSE_FILLED) {  // the whole wave
    const uint32_t g = d.x, k = jcur[m], at = fill[m];
    const uint64_t f = jbase[m >> LINK_SCAN_SHIFT] + jfirst[m];
    for (uint32_t c0 = 0; c0 < g; c0 += 64) {
      const uint32_t c = c0 + lane;
      uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
      for (uint32_t q = 0; q < k; q++) {
        const uint4 s = cands[f + q];  // the same for every lane
        if (s.z != g) continue;
        if (c < g) {
          const uint8_t *p = bases + (s.x | ((uint64_t)s.y << 32));
          uint32_t code = base_code4(s.w ? p[g - 1u - c] : p[c]);  // the index of a voting byte, or 4
          if (s.w && code < 4u) code = 3u - code;  // the complement
          n0 += code == 0u;
          n1 += code == 1u;
          n2 += code == 2u;
          n3 += code == 3u;
        }
      }
      uint32_t best = n0, ch = 'A';
      if (n1 > best) best = n1, ch = 'C';
      if (n2 > best) best = n2, ch = 'G';
      if (n3 > best) best = n3, ch = 'T';
      if (c < g) buf[at + c] = (uint8_t)(best ? ch : (uint32_t)'N');
      disputed += wave_count(c < g && (n0 != 0u) + (n1 != 0u) + (n2 != 0u) + (n3 != 0u) > 1u);
    }
    if (lane == 0 && disputed && closures) ((uint32_t *)(closures + 2 * m + 1))[1] = disputed;
  }
  // one atomic a workgroup of sixteen joins, not one a disputed join: every lane of a wave holds the wave's count
  const int k1[1] = {CLS_DISPUTED};
  const uint32_t mine[1] = {lane == 0 ? disputed : 0u};
  wg_stats<1>(st, k1, mine);
}

// scaffolds, offsets: may be null
__global__ void __launch_bounds__(CLOSE_TPB) kc_close_records_kernel(const uint4 *scaf_in, uint64_t n_scaf, const uint32_t *seg, const uint32_t *acc,
                                                                     uint32_t total, uint4 *scaffolds, uint64_t *offsets) {
  const uint64_t s = (uint64_t)blockIdx.x * CLOSE_TPB + threadIdx.x;
  if (s >= n_scaf) return;
  const uint4 a = scaf_in[2 * s], b = scaf_in[2 * s + 1];
  const uint32_t at = seg[a.x];
  if (offsets) {
    offsets[s] = at;
    if (s == 0) offsets[n_scaf] = total;
  }
  if (scaffolds) {
    scaffolds[2 * s] = make_uint4(a.x, a.y, seg[a.x + a.y] - 1u - at, acc[2 * s]);
    scaffolds[2 * s + 1] = make_uint4(acc[2 * s + 1], b.y, 0u, 0u);
  }
}

// kc_scaffold.hpp's writer, with a filled member's run taken from buf
static_assert(CLOSE_TPB == SCAF_TPB && CLOSE_NONE == SCAF_NONE, "scaf_write_body's workgroup and its mark of a run without fill");
__global__ void __launch_bounds__(CLOSE_TPB) kc_close_write_kernel(const uint4 *members, const uint32_t *seg, const uint32_t *fill, uint32_t n,
                                                                   const uint8_t *src, const uint32_t *offs, const uint8_t *buf, uint32_t mis,
                                                                   uint32_t total, uint8_t *out) {
  scaf_write_body<true>(members, seg, fill, n, src, offs, buf, mis, total, out);
}

}  // namespace kc
