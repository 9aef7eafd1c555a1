// csrc/kc_debug_fill.hpp on the host: the byte KC_DEBUG_FILL names.  The named strings of the variable's range, every
// decimal and hexadecimal spelling of 0..300 (both letter cases, with leading zeros) against the number itself, and
// every one- and two-byte string against a plain restatement of the grammar; then the environment reader on a set and
// an unset variable.  A host build of the header, a program of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mhm2_kmer_analysis_v2_amd/csrc/kc_debug_fill.hpp"

using namespace kc;

static long long cases = 0;
static int bad_count = 0;

static void check(const char *s, int want) {
  cases++;
  const int got = parse_debug_fill(s);
  if (got != want && bad_count++ < 10) std::printf("\"%s\": got %d, want %d\n", s ? s : "(null)", got, want);
}

// the grammar restated: digits only, or 0x and hex digits only; at most 255
static int spec(const char *s) {
  const size_t n = std::strlen(s);
  if (!n) return -1;
  const bool hex = n >= 2 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X');
  const char *d = hex ? s + 2 : s;
  if (!*d) return -1;
  if (std::strspn(d, hex ? "0123456789abcdefABCDEF" : "0123456789") != std::strlen(d)) return -1;
  const unsigned long v = std::strtoul(d, nullptr, hex ? 16 : 10);
  return v <= 255 ? (int)v : -1;
}

int main() {
  check(nullptr, -1);
  check("", -1);
  check("0", 0);
  check("255", 255);
  check("256", -1);
  check("0xA5", 0xA5);
  check("0x5a", 0x5A);
  check("-1", -1);
  check("12x", -1);
  check("0x", -1);
  check("0X5A", 0x5A);
  check(" 1", -1);
  check("1 ", -1);
  check("+1", -1);
  check("0x100", -1);
  check("017", 17);  // decimal, not octal
  check("99999999999999999999999999", -1);  // no overflow on the way to the verdict
  check("0xFFFFFFFFFFFFFFFFFFFFFFFF", -1);
  char buf[32];
  for (int v = 0; v <= 300; v++) {
    const int want = v <= 255 ? v : -1;
    std::snprintf(buf, sizeof(buf), "%d", v), check(buf, want);
    std::snprintf(buf, sizeof(buf), "%05d", v), check(buf, want);
    std::snprintf(buf, sizeof(buf), "0x%x", v), check(buf, want);
    std::snprintf(buf, sizeof(buf), "0x%X", v), check(buf, want);
    std::snprintf(buf, sizeof(buf), "0X%04x", v), check(buf, want);
    std::snprintf(buf, sizeof(buf), "%x", v), check(buf, spec(buf));  // hex digits without the prefix
  }
  for (int a = 1; a < 256; a++) {
    buf[0] = (char)a, buf[1] = 0;
    check(buf, spec(buf));
    for (int b = 1; b < 256; b++) {
      buf[1] = (char)b, buf[2] = 0;
      check(buf, spec(buf));
      buf[2] = '7', buf[3] = 0;
      check(buf, spec(buf));
    }
  }
  cases++;
  unsetenv("KC_DEBUG_FILL");
  if (debug_fill_byte() != -1) bad_count++, std::printf("unset variable: %d\n", debug_fill_byte());
  cases++;
  setenv("KC_DEBUG_FILL", "0xA5", 1);
  if (debug_fill_byte() != 0xA5) bad_count++, std::printf("0xA5 in the environment: %d\n", debug_fill_byte());
  cases++;
  setenv("KC_DEBUG_FILL", "12x", 1);
  if (debug_fill_byte() != -1) bad_count++, std::printf("12x in the environment: %d\n", debug_fill_byte());
  std::printf("cases=%lld bad=%d\n", cases, bad_count);
  return bad_count ? 1 : 0;
}
