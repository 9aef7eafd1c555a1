// The pure helpers of csrc/kc_kit.hpp on the host, against the definitions the kernel headers carried before the kit: the
// two byte functions and the code-to-letter word over every byte, the digit count and the BCD word at the powers of ten
// and the limits of the widths in use (and against snprintf), and the search against a linear scan -- every [lo, hi] of
// strictly increasing arrays of one to nine items, every x from a[lo] to one past a[hi], under both contracts the
// kernels use.  The old definitions stand here as the specification.  A host build: the wave helpers are device code
// and are held to their models by the GPU tests of the kernels that call them.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../mhm2_kmer_analysis_v2_amd/csrc/kc_kit.hpp"

using namespace kc;

static long long cases = 0;
static int bad_count = 0;

static void check(bool ok, const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
  cases++;
  if (!ok && bad_count++ < 10) std::printf("%s: %llu %llu %llu\n", what, a, b, c);
}

// ---- what the headers held -------------------------------------------------------------------------------------------
static uint32_t old_lassm_code(uint32_t ch) {  // kc_lassm.hpp; kc_close.hpp's close_code was the same
  const uint32_t c = ch & 0xDFu;
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
static uint32_t old_scaf_comp(uint32_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }
static uint32_t old_unitig_letter(uint32_t code) { return (0x54474341u >> (8 * code)) & 0xFFu; }
static uint32_t old_asm_id_digits(uint32_t u) {
  return u < 10u ? 1u : u < 100u ? 2u : u < 1000u ? 3u : u < 10000u ? 4u : u < 100000u ? 5u : u < 1000000u ? 6u : u < 10000000u ? 7u
       : u < 100000000u ? 8u : u < 1000000000u ? 9u : 10u;
}
static uint32_t old_dump_count_digits(uint32_t c) { return c < 10 ? 1u : c < 100 ? 2u : c < 1000 ? 3u : c < 10000 ? 4u : 5u; }
static uint32_t old_rtext_digits(uint64_t v) {
  uint32_t d = 1;
  for (uint64_t p = 10; d < 16 && v >= p; p *= 10) d++;
  return d;
}
static uint64_t old_asm_bcd(uint32_t u) {
  uint64_t bcd = 0;
  int s = 0;
  do {
    bcd |= (uint64_t)(u % 10u) << s;
    u /= 10u;
    s += 4;
  } while (u);
  return bcd;
}
static uint64_t old_rtext_bcd(uint64_t v) {
  uint64_t bcd = 0;
  int s = 0;
  do {
    bcd |= (v % 10u) << s;
    v /= 10u;
    s += 4;
  } while (v);
  return bcd;
}
// asm_find, depth_find_ctg, shuf_find_pair, fa_find_line: the greatest j in [lo, hi] with a[j] <= x (a[lo] <= x)
template <class I>
static I old_find(const uint64_t *a, I lo, I hi, uint64_t x) {
  while (lo < hi) {
    const I mid = lo + ((hi - lo + 1) >> 1);
    if (a[mid] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}
// the writers: the first of n segments that starts behind `from`; the one before it holds `from` (a[0] <= from)
static uint32_t old_first_behind(const uint64_t *a, uint32_t n, uint64_t from) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= from)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- the checks ------------------------------------------------------------------------------------------------------
static void bytes() {
  for (uint32_t c = 0; c < 256; c++) {
    check(base_code4(c) == old_lassm_code(c), "base_code4", c, base_code4(c), old_lassm_code(c));
    check(base_comp(c) == old_scaf_comp(c), "base_comp", c, base_comp(c), old_scaf_comp(c));
  }
  for (uint32_t code = 0; code < 4; code++)
    check(code_letter(code) == old_unitig_letter(code) && code_letter(code) == (uint32_t)"ACGT"[code], "code_letter", code, code_letter(code), 0);
}

static void decimal_at(uint64_t v) {
  char text[32];
  const uint32_t len = (uint32_t)std::snprintf(text, sizeof(text), "%" PRIu64, v);
  const uint32_t d16 = dec_digits<16>(v);
  check(d16 == old_rtext_digits(v), "dec_digits<16> against the loop", v, d16, old_rtext_digits(v));
  check(d16 == (len < 16 ? len : 16), "dec_digits<16> against snprintf", v, d16, len);
  if (len <= 16) {
    const uint64_t bcd = dec_bcd(v);
    check(bcd == old_rtext_bcd(v), "dec_bcd (64 bits) against the old one", v, bcd, old_rtext_bcd(v));
    bool same = (len == 16 || (bcd >> (4 * len)) == 0);
    for (uint32_t i = 0; i < len; i++) same = same && ((bcd >> (4 * i)) & 15u) == (uint64_t)(text[len - 1 - i] - '0');
    check(same, "dec_bcd against snprintf", v, bcd, len);
  }
  if (v <= 0xFFFFFFFFull) {
    const uint32_t u = (uint32_t)v;
    check(dec_digits<10>(u) == old_asm_id_digits(u) && dec_digits<10>(u) == len, "dec_digits<10>", v, dec_digits<10>(u), len);
    check(dec_bcd(u) == old_asm_bcd(u) && dec_bcd(u) == dec_bcd(v), "dec_bcd (32 bits)", v, dec_bcd(u), old_asm_bcd(u));
    check(dec_digits<5>(u) == old_dump_count_digits(u), "dec_digits<5> against the chain", v, dec_digits<5>(u), old_dump_count_digits(u));
    if (v <= 65535) check(dec_digits<5>(u) == len, "dec_digits<5> against snprintf", v, dec_digits<5>(u), len);
  }
}

static void decimal() {
  decimal_at(0);
  decimal_at(9);
  decimal_at(10);
  uint64_t p = 1;
  for (int k = 1; k <= 16; k++) {  // 10^k - 1 has k digits, 10^k one more: 10^16 is the first value the BCD word cannot hold
    p *= 10;
    decimal_at(p - 1);
    decimal_at(p);
  }
  decimal_at(65535);
  decimal_at(65536);
  decimal_at(0xFFFFFFFFull);
  decimal_at(0x100000000ull);
  decimal_at(~0ull);
}

static void search() {
  for (uint32_t n = 1; n <= 9; n++)
    for (uint64_t first = 0; first <= 5; first += 5)
      for (uint32_t gaps = 0; gaps < (1u << (n - 1)); gaps++) {  // bit i: the step from item i to item i + 1 is 3, else 1
        uint64_t a[9], twice[18], ends[9];
        a[0] = first;
        for (uint32_t i = 1; i < n; i++) a[i] = a[i - 1] + (((gaps >> (i - 1)) & 1u) ? 3 : 1);
        for (uint32_t i = 0; i < n; i++) {
          twice[2 * i] = a[i];  // kc_shuffle.hpp reads every other entry
          twice[2 * i + 1] = ~0ull;
          if (i) ends[i - 1] = a[i] - 1;  // kc_fasta_in.hpp: item i starts behind the end of item i - 1
        }
        for (uint32_t lo = 0; lo < n; lo++)
          for (uint32_t hi = lo; hi < n; hi++)
            for (uint64_t x = a[lo]; x <= a[hi] + 1; x++) {
              uint32_t want = lo;
              for (uint32_t j = lo; j <= hi; j++)
                if (a[j] <= x) want = j;
              const uint32_t g32 = find_le(a, lo, hi, x);
              const uint64_t g64 = find_le(a, (uint64_t)lo, (uint64_t)hi, x);
              const uint64_t gs = find_le((uint64_t)lo, (uint64_t)hi, x, [&](uint64_t mid) { return twice[2 * mid]; });
              const uint64_t ge = find_le((uint64_t)lo, (uint64_t)hi, x, [&](uint64_t mid) { return ends[mid - 1] + 1; });
              check(g32 == want && g64 == want && gs == want && ge == want, "find_le against the scan", n * 100 + lo * 10 + hi, x, g32);
              check(g32 == old_find(a, lo, hi, x) && g64 == old_find(a, (uint64_t)lo, (uint64_t)hi, x), "find_le against the old loop", n, x, g32);
            }
        // the writers' contract: a[0] <= x, the first of the n items that starts behind x (n: none does)
        for (uint64_t x = a[0]; x <= a[n - 1] + 1; x++) {
          uint32_t want = n;
          for (uint32_t j = n; j-- > 0;)
            if (a[j] > x) want = j;
          const uint32_t got = find_le(a, 0u, n - 1u, x) + 1u;
          check(got == want && got == old_first_behind(a, n, x), "find_le + 1 against the first item behind x", n, x, got);
        }
      }
}

int main() {
  bytes();
  decimal();
  search();
  std::printf("cases=%lld bad=%d\n", cases, bad_count);
  return bad_count != 0;
}
