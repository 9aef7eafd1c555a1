// kc_debug_fill.hpp -- KC_DEBUG_FILL=<byte>: the byte a fresh allocation of the library is filled with, so that a result
// that depends on memory the library has not written shows ("Poisoned scratch").  Host-compilable and on its
// own (tests/cpp/test_debug_fill.cpp); kc_api_mem.hpp reads the variable through it at allocation time.
#pragma once
#include <stdlib.h>

namespace kc {

// The byte `s` names, or -1 for none: decimal ("165") or hexadecimal behind 0x / 0X ("0xA5"), 0..255, the whole string and
// nothing else (no sign, no blank, no octal reading of a leading 0).  nullptr, "" and anything else: -1.
inline int parse_debug_fill(const char *s) {
  if (!s || !*s) return -1;
  int base = 10;
  if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) base = 16, s += 2;
  if (!*s) return -1;
  int v = 0;
  for (; *s; s++) {
    int d;
    if (*s >= '0' && *s <= '9') d = *s - '0';
    else if (base == 16 && *s >= 'a' && *s <= 'f') d = *s - 'a' + 10;
    else if (base == 16 && *s >= 'A' && *s <= 'F') d = *s - 'A' + 10;
    else return -1;
    v = v * base + d;
    if (v > 255) return -1;
  }
  return v;
}

// ... of the environment, read anew at every call (like KC_HOST_BLOCK): unset costs the getenv and nothing else
inline int debug_fill_byte() { return parse_debug_fill(getenv("KC_DEBUG_FILL")); }

}  // namespace kc
