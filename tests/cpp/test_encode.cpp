// The word-parallel staging of a sixteen-byte group (encode_group_swar, encode_group_codes: csrc/kc_encode.hpp) on the
// host against the byte-by-byte form the kernels keep for the edges of the data (encode_group_edge) and kc_base_code:
// every base byte x every quality byte in each of the sixteen positions of a group, the other fifteen bytes valid, for
// the quality cuts 33, 53 and 128 and the three input formats.  Codes, ok bits, separator bits and `bad` must agree bit
// for bit.
// A host build: kc_udot4, kc_perm4 and kc_wave_any run their host fallbacks here.  The device builtins behind them (the operand
// order of the byte permute, the wave-wide branch with lanes that disagree) are exercised only on the GPU, by
// tests/test_gpu_l1_staging_copy_out.py.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../mhm2_kmer_analysis_v2_amd/csrc/kc_encode.hpp"

using namespace kc;

static long long cases = 0;
static int bad_count = 0;

static void words(const uint8_t (&b)[16], uint32_t (&w)[4]) {
  for (int j = 0; j < 4; j++) w[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
}

template <int FMT>
static uint32_t codes_by_byte(const uint8_t (&b)[16]) {
  uint32_t code = 0;
  for (int i = 0; i < 16; i++) {
    const uint32_t c = b[i];
    const uint32_t x = FMT == FMT_PACKED ? ((c & 3u) | ((c >> 1) & 2u)) : kc_base_code(c);  // cache bytes: base 0-4 = ACGTN, N -> G
    code |= x << (30 - 2 * i);
  }
  return code;
}

template <int FMT>
static void one(const uint8_t (&b)[16], const uint8_t (&q)[16], int qual_cut) {
  uint32_t bw[4], qw[4];
  words(b, bw);
  words(q, qw);
  uint32_t ok_e = 0, sep_e = 0, ok_s = 0, sep_s = 0;
  bool bad_e = false, bad_s = false;
  encode_group_edge<FMT>(bw, qw, qual_cut, 0, 0, 16, ok_e, sep_e, bad_e);
  encode_group_swar<FMT>(bw, qw, (uint32_t)qual_cut, ok_s, sep_s, bad_s);
  const uint32_t code_e = codes_by_byte<FMT>(b), code_s = encode_group_codes<FMT>(bw);
  cases++;
  if (ok_e != ok_s || sep_e != sep_s || bad_e != bad_s || code_e != code_s) {
    if (bad_count++ < 10) {
      std::printf("fmt %d cut %d bases", FMT, qual_cut);
      for (int i = 0; i < 16; i++) std::printf(" %02x", b[i]);
      std::printf(" quals");
      for (int i = 0; i < 16; i++) std::printf(" %02x", q[i]);
      std::printf(": ok %04x/%04x sep %04x/%04x bad %d/%d codes %08x/%08x\n", ok_e, ok_s, sep_e, sep_s, (int)bad_e, (int)bad_s, code_e, code_s);
    }
  }
}

// the fifteen other bytes: valid ones of every kind the format has
template <int FMT>
static void background(int which, int qual_cut, uint8_t (&b)[16], uint8_t (&q)[16]) {
  static const char *ascii[3] = {"ACGTACGTACGTACGT", "acgtNnTGCAtgcaGg", "TTgNAcCaGGtTnACg"};
  static const char *block[3] = {"ACGTACGTACGTACGT", "acgt_nTGCA_gcaGg", "T_gNAcCaGGtTnAC_"};
  for (int i = 0; i < 16; i++) {
    if (FMT == FMT_PACKED) {
      const uint32_t base = (uint32_t)((i * 7 + which * 3) % 5), qual = (uint32_t)((i * 11 + which * 13) % 32);
      b[i] = (uint8_t)(base | (qual << 3));
      q[i] = 0;
    } else {
      b[i] = (uint8_t)(FMT == FMT_SEQBLOCK ? block[which][i] : ascii[which][i]);
      const int qs[5] = {qual_cut - 1, qual_cut, qual_cut + 1, 33, 126};
      q[i] = (uint8_t)(which == 0 ? 126 : qs[(i + which) % 5]);
    }
  }
}

template <int FMT>
static void sweep() {
  const int cuts[3] = {33, 53, 128};
  for (int ci = 0; ci < (FMT == FMT_READS ? 3 : 1); ci++)
    for (int which = 0; which < 3; which++) {
      uint8_t b0[16], q0[16];
      background<FMT>(which, cuts[ci], b0, q0);
      for (int pos = 0; pos < 16; pos++)
        for (int c = 0; c < 256; c++)
          for (int qq = 0; qq < (FMT == FMT_READS ? 256 : 1); qq++) {
            uint8_t b[16], q[16];
            std::memcpy(b, b0, 16);
            std::memcpy(q, q0, 16);
            b[pos] = (uint8_t)c;
            if (FMT == FMT_READS) q[pos] = (uint8_t)qq;
            one<FMT>(b, q, cuts[ci]);
          }
    }
}

int main() {
  sweep<FMT_READS>();
  sweep<FMT_SEQBLOCK>();
  sweep<FMT_PACKED>();
  // two and sixteen bytes outside the alphabet at once, and all sixteen the same byte
  for (int c = 0; c < 256; c++) {
    uint8_t b[16], q[16];
    for (int i = 0; i < 16; i++) { b[i] = (uint8_t)c; q[i] = (uint8_t)(40 + i); }
    one<FMT_READS>(b, q, 53);
    one<FMT_SEQBLOCK>(b, q, 53);
    one<FMT_PACKED>(b, q, 53);
    for (int d = 0; d < 256; d++) {
      for (int i = 0; i < 16; i++) b[i] = (uint8_t)"ACGT"[i & 3];
      b[3] = (uint8_t)c;
      b[4] = (uint8_t)d;
      one<FMT_READS>(b, q, 53);
      one<FMT_SEQBLOCK>(b, q, 53);
    }
  }
  std::printf("cases=%lld bad=%d\n", cases, bad_count);
  return bad_count != 0;
}
