// kc_api_sort.hpp -- the results' back end of the C ABI: kc_sort_results and kc_dump_text_device (kernels in
// kc_sort.hpp).  Part of kc_api.hip's translation unit, like kc_api_frontend.hpp.

// the passes of the sort: (word, shift, bits), from the least significant digit of the last word up
struct SortPass {
  int w, shift, bits;
};

static std::vector<SortPass> sort_passes(int k, int nl_ext) {
  std::vector<SortPass> v;
  for (int w = nl_ext - 1; w >= 0; w--) {
    const int sig = std::min(64, 2 * k - 64 * w);  // significant bits, at the top of the word (S3); none: no pass
    for (int shift = 64 - std::max(sig, 0); shift < 64; shift += SORT_BITS) v.push_back({w, shift, std::min(SORT_BITS, 64 - shift)});
  }
  return v;
}

// the results in key order in fresh arrays of the call's (ext: the keys at the reference's width, where that differs)
struct Sorted {
  uint64_t *keys, *ext;
  uint16_t *counts;
  uint8_t *left, *right;
};

static int sort_run(kc_ctx *c, CallBufs &cb, Sorted &b) {
  const uint64_t n = c->out_n;
  const uint64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE;
  const uint64_t ncnt = ntiles * SORT_DIGITS;
  const bool two = c->nl != c->nl_ext;
  KCTRY(cb.alloc(&b.keys, n * c->nl * 8));
  KCTRY(cb.alloc(&b.ext, two ? n * c->nl_ext * 8 : 0));
  KCTRY(cb.alloc(&b.counts, n * 2));
  KCTRY(cb.alloc(&b.left, n));
  KCTRY(cb.alloc(&b.right, n));
  uint64_t *kbuf[2], *cnt, *total;
  uint32_t *ibuf[2];
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    kbuf[0] = m.take<uint64_t>(n);
    kbuf[1] = m.take<uint64_t>(n);
    ibuf[0] = m.take<uint32_t>(n);
    ibuf[1] = m.take<uint32_t>(n);
    cnt = m.take<uint64_t>(ncnt);
    total = m.take<uint64_t>(1);
    return m.used;
  };
  KCTRY(cb.carve(layout));
  // the order is that of the keys at the reference's width: its words are the first nl_ext of the library's
  const uint64_t *keys = c->d_out_keys;
  const uint32_t *perm = nullptr;  // the identity until the first pass has run
  int cur = 0, loaded = -1;
  for (const SortPass &p : sort_passes(c->k, c->nl_ext)) {
    const uint32_t mask = (1u << p.bits) - 1u;
    if (p.w != loaded) {
      KCTRY(launch_timed(c, KT_SORT_HIST_LOAD, kc_sort_hist_kernel<true>, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, keys, c->nl, p.w, perm,
                         kbuf[cur], n, ntiles, p.shift, mask, cnt));
      loaded = p.w;
    } else {
      KCTRY(launch_timed(c, KT_SORT_HIST, kc_sort_hist_kernel<false>, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, keys, c->nl, p.w, perm,
                         kbuf[cur], n, ntiles, p.shift, mask, cnt));
    }
    KCTRY(launch_timed(c, KT_SORT_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{cnt}}, ncnt, total));
    KCTRY(launch_timed(c, KT_SORT_SCATTER, kc_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)kbuf[cur], perm,
                       kbuf[cur ^ 1], ibuf[cur ^ 1], n, ntiles, p.shift, mask, (const uint64_t *)cnt));
    cur ^= 1;
    perm = ibuf[cur];
  }
  if (!perm) {  // k-mers without a significant bit do not exist (k >= 3), but an identity is still an order
    HIPCHK(hipMemcpyAsync(b.keys, c->d_out_keys, n * c->nl * 8, hipMemcpyDeviceToDevice, c->stream));
    if (two) HIPCHK(hipMemcpyAsync(b.ext, c->d_out_keys_ext, n * c->nl_ext * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.counts, c->d_out_counts, n * 2, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.left, c->d_out_left, n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.right, c->d_out_right, n, hipMemcpyDeviceToDevice, c->stream));
  } else {
    KCTRY(launch_timed(c, KT_SORT_GATHER, kc_sort_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, perm, n, c->nl,
                       (const uint64_t *)c->d_out_keys, b.keys, c->nl_ext, (const uint64_t *)(two ? c->d_out_keys_ext : nullptr), b.ext,
                       (const uint16_t *)c->d_out_counts, b.counts, (const uint8_t *)c->d_out_left, b.left, (const uint8_t *)c->d_out_right,
                       b.right));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

static void fill_result(const kc_ctx *c, kc_result *out) {
  out->n = c->out_n;
  out->num_longs = c->nl_ext;
  out->reserved = 0;
  out->d_keys = c->nl != c->nl_ext ? c->d_out_keys_ext : c->d_out_keys;
  out->d_counts = c->d_out_counts;
  out->d_left = c->d_out_left;
  out->d_right = c->d_out_right;
}

extern "C" int kc_sort_results(kc_ctx *c, kc_result *out) {
  if (!c) return KC_ERR_INVALID_ARG;
  if (!c->finalized) return KC_ERR_STATE;
  if (!c->sorted && c->out_n > 1) {
    if (c->out_n >= (1ull << 32))
      return fail(KC_ERR_CAPACITY, "kc_sort_results: %llu results, the permutation is 32-bit (fewer than 2^32)", (unsigned long long)c->out_n);
    KCTRY(call_with_bufs(c, [&](CallBufs &cb) {
      Sorted b;
      KCTRY(sort_run(c, cb, b));  // had it failed, the unsorted results would be as they were
      free_index(c);  // it holds positions: the next kc_lookup builds it over the new order
      cb.hand_over(b.keys, c->d_out_keys);  // the old arrays go
      if (b.ext) cb.hand_over(b.ext, c->d_out_keys_ext);
      cb.hand_over(b.counts, c->d_out_counts);
      cb.hand_over(b.left, c->d_out_left);
      cb.hand_over(b.right, c->d_out_right);
      c->out_cap = c->out_n;
      return (int)KC_OK;
    }));
  }
  c->sorted = true;
  if (out) fill_result(c, out);
  return KC_OK;
}

extern "C" int kc_dump_text_device(kc_ctx *c, uint64_t first, uint64_t count, uint8_t *d_text, uint64_t capacity, uint64_t *nbytes) {
  if (!c || !nbytes) return KC_ERR_INVALID_ARG;
  *nbytes = 0;
  if (!c->finalized) return KC_ERR_STATE;
  if (first > c->out_n || count > c->out_n - first) return KC_ERR_INVALID_ARG;
  if (!count) return KC_OK;
  const uint64_t ntiles = (count + DUMP_TILE - 1) / DUMP_TILE;
  if (ntiles > 0x7FFFFFFFull) return fail(KC_ERR_CAPACITY, "kc_dump_text_device: at most 2^31 - 1 tiles of %d lines a call", DUMP_TILE);
  HIPCHK(hipSetDevice(c->cfg.device));
  KCTRY(c->dump_tiles.reserve((ntiles + 1) * 8));
  uint64_t *tiles = c->dump_tiles.as<uint64_t>(), *total = tiles + ntiles;
  KCTRY(launch_timed(c, KT_DUMP_SIZES, kc_dump_sizes_kernel, dim3((unsigned)ntiles), dim3(DUMP_TILE), 0, (const uint16_t *)c->d_out_counts, first,
                     count, c->k, tiles));
  KCTRY(launch_timed(c, KT_DUMP_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{tiles}}, ntiles, total));
  uint64_t tot = 0;
  HIPCHK(hipMemcpyAsync(&tot, total, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *nbytes = tot;
  if (!d_text) return KC_OK;  // a size query
  if (tot > capacity)
    return fail(KC_ERR_CAPACITY, "kc_dump_text_device: %llu lines are %llu bytes, the buffer holds %llu", (unsigned long long)count,
                (unsigned long long)tot, (unsigned long long)capacity);
  const uint64_t *keys = c->nl != c->nl_ext ? c->d_out_keys_ext : c->d_out_keys;
  KCTRY(launch_timed(c, KT_DUMP_WRITE, kc_dump_write_kernel, dim3((unsigned)ntiles), dim3(DUMP_TILE), 0, keys, c->nl_ext,
                     (const uint16_t *)c->d_out_counts, (const uint8_t *)c->d_out_left, (const uint8_t *)c->d_out_right, first, count, c->k,
                     (const uint64_t *)tiles, d_text));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}
