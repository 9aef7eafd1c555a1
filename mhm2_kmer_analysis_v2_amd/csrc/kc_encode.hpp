// kc_encode.hpp -- sixteen input bytes -> 2-bit codes, "may serve as an extension" bits, separator bits and the
// bad-byte flag of a staged tile (S2, S3, S5), for host and device: the kernels' tile staging (kc_kernels.hpp,
// tile_encode_fill) calls the two forms below, tests/cpp/test_encode.cpp holds one against the other on the host.
//
//   encode_group_edge   byte by byte, bytes outside the data masked: the specification
//   encode_group_swar   four bytes per instruction, for a group whose sixteen bytes are all real data
#pragma once
#include "kc_common.hpp"

namespace kc {

// input formats: ASCII bases + qualities; the reference's '_'-joined case-masked block; the reference's read
// cache bytes (3-bit base | 5-bit quality << 3, src/packed_reads.cpp:99-126)
// FMT_READS_UQ: FMT_READS whose quality array is not 16-byte co-aligned with the base array (its own
// instantiation: the byte loads it needs would otherwise cost the common case registers)
enum { FMT_READS = 0, FMT_SEQBLOCK = 1, FMT_PACKED = 2, FMT_READS_UQ = 3 };
constexpr bool fmt_is_reads(int fmt) { return fmt == FMT_READS || fmt == FMT_READS_UQ; }

// ---- the three machine operations the word-parallel form leans on, with host fallbacks ---------------------------
// sum of the four byte products + c
KC_HD uint32_t kc_udot4(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  for (int i = 0; i < 4; i++) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return c;
#endif
}
// byte i of the result = byte sel[i] of the constant tab (selector bytes 0..3 only)
template <uint32_t tab>
KC_HD uint32_t kc_perm4(uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (the table in a scalar register: as a vector register, the compiler's choice, it is set up once in front of a kernel's
  // main loop and occupies a register through all of it)
  uint32_t t;
  asm("s_mov_b32 %0, %1" : "=s"(t) : "i"(tab));
  return __builtin_amdgcn_perm(0u, t, sel);
#else
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) r |= ((tab >> (8 * ((sel >> (8 * i)) & 3u))) & 0xFFu) << (8 * i);
  return r;
#endif
}
// true in every lane of the wave if it is true in one (the host has one lane)
KC_HD bool kc_wave_any(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __any(x) != 0;
#else
  return x;
#endif
}

// ---- 2-bit codes ---------------------------------------------------------------------------------------------------
// Bits 2:1 of an ASCII base are its code in Gray form (A0 C1 T2 G3, N as G; case does not reach them); code = g ^ (g >> 1)
// (kc_base_code).  The sixteen Gray forms are gathered first, one dot product per word with the weights 64, 16, 4, 1
// (first byte highest), and turned into codes all at once.
constexpr uint32_t GATHER2 = 0x01041040u;
KC_HD uint32_t gray4(uint32_t v) { return (v >> 1) & 0x03030303u; }  // 4 ASCII bytes -> their Gray forms, one a byte
KC_HD uint32_t pack16(const uint32_t (&bw)[4]) {  // 16 ASCII bytes -> 16 codes, first byte highest
  // (four independent dot products: a result chained through a shift into the next one's addend waits for it each time)
  const uint32_t g0 = kc_udot4(gray4(bw[0]), GATHER2, 0u), g1 = kc_udot4(gray4(bw[1]), GATHER2, 0u);
  const uint32_t g2 = kc_udot4(gray4(bw[2]), GATHER2, 0u), g3 = kc_udot4(gray4(bw[3]), GATHER2, 0u);
  const uint32_t g = (g0 << 24) | (g1 << 16) | (g2 << 8) | g3;
  return g ^ ((g >> 1) & 0x55555555u);
}
KC_HD uint32_t pack4_cache(uint32_t v) {  // 4 read-cache bytes (base 0-4 = ACGTN) -> 4 codes, N -> G
  return kc_udot4((v & 0x03030303u) | ((v >> 1) & 0x02020202u), GATHER2, 0u);
}
KC_HD uint32_t pack16_cache(const uint32_t (&bw)[4]) {
  return (pack4_cache(bw[0]) << 24) | (pack4_cache(bw[1]) << 16) | (pack4_cache(bw[2]) << 8) | pack4_cache(bw[3]);
}
template <int FMT>
KC_HD uint32_t encode_group_codes(const uint32_t (&bw)[4]) {
  return FMT == FMT_PACKED ? pack16_cache(bw) : pack16(bw);
}

constexpr uint32_t BM_ACGT = (1u << 1) | (1u << 3) | (1u << 7) | (1u << 20);
constexpr uint32_t BM_ACGTN = BM_ACGT | (1u << 14);
KC_HD bool in_bitmap(uint32_t c, uint32_t bm) { return ((c & 0xC0u) == 0x40u) && ((bm >> (c & 31u)) & 1u); }

// ---- byte by byte --------------------------------------------------------------------------------------------------
// S2/S5 for any group: byte i of the group has aligned coordinate X0 + i, real data is [lo, hi).  okm bit i = byte i may
// serve as an extension, sepm bit i = byte i is a separator (FMT_SEQBLOCK), bad |= a byte outside the alphabet
template <int FMT>
KC_HD void encode_group_edge(const uint32_t (&bw)[4], const uint32_t (&qw)[4], int qual_cut, int64_t X0, int64_t lo, int64_t hi,
                             uint32_t &okm, uint32_t &sepm, bool &bad) {
  const bool any = (X0 + 16 > lo) && (X0 < hi);
  const bool full = (X0 >= lo) && (X0 + 16 <= hi);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t wb = bw[j], wq = qw[j];
#pragma unroll 1
    for (int i = 4 * j; i < 4 * j + 4; i++, wb >>= 8, wq >>= 8) {
      const uint32_t c = wb & 0xFFu;
      const bool real = full || (any && (X0 + i >= lo) && (X0 + i < hi));
      bool hq;
      if (FMT == FMT_PACKED) {
        hq = (c >> 3) >= KC_QUAL_CUTOFF;                      // S2 on the stored quality (already relative to qual_offset)
        if (real && (c & 7u) > 4u) bad = true;
        if (real && hq && (c & 7u) < 4u) okm |= 1u << i;
        continue;
      }
      if (fmt_is_reads(FMT)) {
        const int q = (int)(wq & 0xFFu);
        hq = q >= qual_cut;                                   // S2
        if (real && !in_bitmap(c, BM_ACGTN)) bad = true;
      } else {
        hq = (c & 0x20u) == 0;                                // case carries the quality
        const bool sep = (c == '_');
        if (real && sep) sepm |= 1u << i;
        if (real && !sep && !in_bitmap(c, BM_ACGTN)) bad = true;
      }
      if (real && hq && in_bitmap(c, BM_ACGT)) okm |= 1u << i;
    }
  }
}

// ---- sixteen bytes at a time -----------------------------------------------------------------------------------
// Byte-parallel predicates: a result word carries its answer in bit 7 of every byte, the other bits are garbage
// until the final gather.  nz7(x): bit 7 set where the byte of x is not zero.
KC_HD uint32_t nz7(uint32_t x) { return ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x; }
// bit 7 set where the byte of w is none of ACGTacgt: the Gray form of a byte selects the one letter it could be
// ('A', 'C', 'T', 'G' for 0, 1, 2, 3), and the byte, upper-cased, either is that letter or is no base
KC_HD uint32_t not_acgt7(uint32_t w) { return nz7((w & 0xDFDFDFDFu) ^ kc_perm4<0x47544341u>(gray4(w))); }

// S2/S5 for a group whose sixteen bytes are all real data (qual_cut <= 128): the same okm, sepm and bad as encode_group_edge's.
// Nearly every group is ACGT throughout, so 'N' and '_' are looked for only where some lane of the wave holds another
// byte (a wave-uniform branch around register arithmetic).
template <int FMT>
KC_HD void encode_group_swar(const uint32_t (&bw)[4], const uint32_t (&qw)[4], uint32_t qual_cut, uint32_t &okm, uint32_t &sepm,
                             bool &bad) {
  // one word after the other, each folded into the running gathers at once (few values live at a time)
  uint32_t badacc = 0, ok_lo = 0, ok_hi = 0;
  const uint32_t cut4 = qual_cut * 0x01010101u;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t w = bw[j];
    const uint32_t weight = (j & 1) ? 0x80402010u : 0x08040201u;  // byte i of the half-group -> bit i (times 0x80)
    uint32_t ok;
    if (FMT == FMT_PACKED) {
      // base = low 3 bits (0-4), quality = high 5: quality >= 20 <=> byte >= 0xA0; base > 4 <=> bit2 & (bit1 | bit0)
      const uint32_t x = w & ((w << 1) | (w << 2));  // bit 7: high quality, bit 2: bad base code
      badacc |= x << 5;
      ok = x & ~(w << 5);                            // high quality and base < 4
    } else {
      const uint32_t na = not_acgt7(w);
      uint32_t hq;
      if (fmt_is_reads(FMT)) {
        const uint32_t q = qw[j];
        hq = (((q & 0x7F7F7F7Fu) | 0x80808080u) - cut4) | q;  // S2: byte >= qual_cut (<= 128)
      } else {
        hq = ~(w << 2);                                       // case carries the quality: bit 5 clear
      }
      badacc |= na;  // (until the branch below has looked: some byte is not ACGT)
      ok = hq & ~na;
    }
    if (j < 2) ok_lo = kc_udot4(ok & 0x80808080u, weight, ok_lo);
    else ok_hi = kc_udot4(ok & 0x80808080u, weight, ok_hi);
  }
  okm = (ok_lo >> 7) | ((ok_hi >> 7) << 8);
  if (FMT == FMT_PACKED) {
    if (badacc & 0x80808080u) bad = true;
  } else if (kc_wave_any((badacc & 0x80808080u) != 0)) {
    uint32_t sp_lo = 0, sp_hi = 0;
    badacc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t w = bw[j];
      const uint32_t weight = (j & 1) ? 0x80402010u : 0x08040201u;
      uint32_t other = not_acgt7(w) & nz7((w & 0xDFDFDFDFu) ^ 0x4E4E4E4Eu);  // neither ACGT nor N
      if (FMT == FMT_SEQBLOCK) {
        const uint32_t not_sep = nz7(w ^ 0x5F5F5F5Fu);
        other &= not_sep;
        if (j < 2) sp_lo = kc_udot4(~not_sep & 0x80808080u, weight, sp_lo);
        else sp_hi = kc_udot4(~not_sep & 0x80808080u, weight, sp_hi);
      }
      badacc |= other;
    }
    if (FMT == FMT_SEQBLOCK) sepm = (sp_lo >> 7) | ((sp_hi >> 7) << 8);
    if (badacc & 0x80808080u) bad = true;
  }
}

}  // namespace kc
