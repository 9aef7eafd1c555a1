// kc_api_fastq_out.hpp -- kc_fastq_text (kernels in kc_fastq_out.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_asm.hpp; the scan is kc_api_call.hpp's, the span table kc_asm.hpp's.

static_assert(sizeof(kc_fastq_out_params) == 64, "the header's layout");
static_assert(KC_FASTQ_OUT_MAX_PREFIX == RTEXT_MAX_PREFIX, "the header's limit is the kernels'");

static int rtext_run(kc_ctx *c, CallBufs &b, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads, const uint32_t *order,
                     uint64_t n_order, const uint64_t *ids, int on_device, const kc_fastq_out_params &prm, uint64_t first_byte, uint8_t *text,
                     uint64_t capacity, uint64_t *written, uint64_t *total) {
  const bool dev = on_device != 0, packed = (prm.flags & KC_FASTQ_OUT_PACKED) != 0, check = (prm.flags & KC_FASTQ_OUT_CHECK) != 0;
  if ((prm.flags & KC_FASTQ_OUT_PAIRED) && (nreads & 1))
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: KC_FASTQ_OUT_PAIRED with %llu reads, an odd number", (unsigned long long)nreads);
  const uint64_t tiles = (n_order + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  RtextArgs a;
  memset(&a, 0, sizeof(a));
  uint8_t *d_prefix;
  StagedIn<uint64_t> offs = staged_offsets(offsets, nreads, dev);
  StagedIn<uint32_t> ord{order, dev, (size_t)n_order * 4, order != nullptr};
  StagedIn<uint64_t> idn{ids, dev, (size_t)nreads * 8, ids != nullptr};
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(RT_COUNT);
    d_prefix = m.take<uint8_t>(RTEXT_MAX_PREFIX);
    a.rs = m.take<uint64_t>(n_order + 1);
    a.rbase = m.take<uint64_t>(tiles);
    a.first_j = check && order ? m.take<uint32_t>(nreads) : nullptr;
    offs.reserve(m, nreads != 0);
    ord.reserve(m, order != nullptr);
    idn.reserve(m, ids != nullptr);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(ord.upload(c));
  KCTRY(idn.upload(c));
  HIPCHK(hipMemcpyAsync(d_prefix, prm.prefix, RTEXT_MAX_PREFIX, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(a.st, 0, RT_BAD_ORDER * 8, c->stream));
  HIPCHK(hipMemsetAsync(a.st + RT_BAD_ORDER, 0xFF, (RT_COUNT - RT_BAD_ORDER) * 8, c->stream));
  if (a.first_j && nreads) HIPCHK(hipMemsetAsync(a.first_j, 0xFF, nreads * 4, c->stream));
  a.offs = nreads ? offs.d : nullptr;
  a.nreads = nreads;
  a.order = order ? ord.d : nullptr;
  a.n_order = n_order;
  a.ids = ids ? idn.d : nullptr;
  a.first_id = prm.first_id;
  a.prefix = d_prefix;
  a.prefix_len = prm.prefix_len;
  a.paired = (prm.flags & KC_FASTQ_OUT_PAIRED) ? 1u : 0u;
  a.qual_splat = ((uint32_t)c->cfg.qual_offset & 0xFFu) * 0x01010101u;
  a.first_byte = first_byte;
  const dim3 tpb(RTEXT_TPB);
  // ---- the checks: their verdict is read before a size is formed from an offset, an order entry or a number
  uint64_t h[RT_COUNT], last = 0;
  memset(h, 0, sizeof(h));
  h[RT_BAD_ORDER] = h[RT_BAD_NUMBER] = h[RT_BAD_J] = ~0ull;
  if (nreads || n_order) {
    KCTRY(launch_timed(c, KT_RTEXT_CHECK, kc_rtext_check_kernel, blocks_for(std::max(nreads + 1, n_order), RTEXT_TPB), tpb, 0, a));
    if (nreads) HIPCHK(hipMemcpyAsync(&last, offs.d + nreads, 8, hipMemcpyDeviceToHost, c->stream));
    KCTRY(read_back(c, h, a.st));
  }
  if (h[RT_BAD_OFFSETS])
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: the offsets of %llu reads do not start at 0 or decrease", (unsigned long long)nreads);
  if (h[RT_TOO_LONG]) return fail(KC_ERR_CAPACITY, "kc_fastq_text: a read of 2^32 bytes or more, positions in a read take 32 bits");
  if (h[RT_BAD_ORDER] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: order[%llu] names no read (%llu reads)", (unsigned long long)h[RT_BAD_ORDER],
                (unsigned long long)nreads);
  if (h[RT_BAD_NUMBER] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: the number of record %llu has more than 16 digits", (unsigned long long)h[RT_BAD_NUMBER]);
  if (last && !bases) return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: bases is NULL and the reads hold %llu bytes", (unsigned long long)last);
  // ---- the reads, sized by checked offsets
  a.nbytes = last;
  a.bases = bases;
  a.quals = packed ? nullptr : quals;
  if (!dev && last) {
    KCTRY(upload_reads(c, b, bases, last, &a.bases));
    if (!packed) KCTRY(upload_reads(c, b, quals, last, &a.quals));
  }
  if (check && n_order && last) {
    KCTRY(launch_timed(c, KT_RTEXT_BYTES, kc_rtext_bytes_kernel, dim3(blocks_for((last + 15 + 15) / 16, RTEXT_TPB).x, packed ? 1 : 2), tpb, 0, a));
    KCTRY(read_back(c, h + RT_BAD_J, a.st + RT_BAD_J, 1));
    if (h[RT_BAD_J] != ~0ull) {
      KCTRY(launch_timed(c, KT_RTEXT_DETAIL, kc_rtext_detail_kernel, dim3(1), tpb, 0, a, h[RT_BAD_J]));
      KCTRY(read_back(c, h, a.st));
      return fail(KC_ERR_BAD_BASE, "kc_fastq_text: record %llu (read %u): %s %llu is 0x%02x, %s", (unsigned long long)h[RT_BAD_J],
                  (unsigned)h[RT_BAD_READ], (h[RT_BAD_KEY] >> 32) ? "quality" : "base", (unsigned long long)(h[RT_BAD_KEY] & 0xFFFFFFFFull),
                  (unsigned)h[RT_BAD_BYTE], packed ? "a code over 4" : "outside 0x21 .. 0x7e");
    }
  }
  // ---- the records' starts and the total
  uint64_t all = 0;
  if (n_order) {
    KCTRY(launch_timed(c, KT_RTEXT_SIZES, kc_rtext_sizes_kernel, blocks_for(n_order, RTEXT_TPB), tpb, 0, a));
    KCTRY(tiled_scan(c, KT_RTEXT_TILE_SCAN, KT_RTEXT_SCAN, a.rs, n_order, a.rbase, a.st + RT_TOTAL));
    KCTRY(launch_timed(c, KT_RTEXT_STARTS, kc_rtext_starts_kernel, blocks_for(n_order + 1, RTEXT_TPB), tpb, 0, a));
    KCTRY(read_back(c, &all, a.st + RT_TOTAL, 1));
  }
  if (first_byte > all)
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: first_byte %llu is behind the text's %llu bytes", (unsigned long long)first_byte,
                (unsigned long long)all);
  const uint64_t n = text ? std::min(all - first_byte, capacity) : 0;
  if (n) {
    // ---- the window
    const uint64_t nspans = (n + (1ull << ASM_SPAN_SHIFT) - 1) >> ASM_SPAN_SHIFT;
    uint32_t *tab;
    uint8_t *d_text = text;
    KCTRY(b.alloc(&tab, nspans * 4));
    if (!dev) KCTRY(b.alloc(&d_text, n));
    a.tab = tab;
    a.text = d_text;
    a.written = n;
    KCTRY(launch_timed(c, KT_RTEXT_SPANS, kc_asm_spans_kernel, blocks_for(nspans, ASM_TPB), dim3(ASM_TPB), 0, (const uint64_t *)a.rs, n_order, first_byte,
                       nspans, tab));
    const uint64_t chunks = (n + 15 + 15) / 16;  // a misaligned array's first chunk is partial
    KCTRY(launch_timed(c, KT_RTEXT_WRITE, kc_rtext_write_kernel, blocks_for(chunks, RTEXT_TPB), tpb, 0, a));
    if (!dev) HIPCHK(hipMemcpyAsync(text, d_text, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  *written = n;
  *total = all;
  return KC_OK;
}

extern "C" int kc_fastq_text(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads, const uint32_t *order,
                             uint64_t n_order, const uint64_t *ids, int on_device, const kc_fastq_out_params *p, uint64_t first_byte, uint8_t *text,
                             uint64_t capacity, uint64_t *written, uint64_t *total) {
  // the ranges come before the context so that they can be checked where there is no device
  constexpr uint32_t known = KC_FASTQ_OUT_PACKED | KC_FASTQ_OUT_PAIRED | KC_FASTQ_OUT_CHECK;
  if (!p || !written || !total) return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: %s is NULL", !p ? "params" : !written ? "written" : "total");
  if (p->flags & ~known) return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: unknown flags 0x%x", p->flags & ~known);
  for (int i = 0; i < 4; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (p->prefix_len > KC_FASTQ_OUT_MAX_PREFIX)
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: prefix_len %u over %d", p->prefix_len, KC_FASTQ_OUT_MAX_PREFIX);
  for (uint32_t i = 0; i < p->prefix_len; i++)
    if ((uint8_t)p->prefix[i] < 0x21 || (uint8_t)p->prefix[i] > 0x7E)
      return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: prefix[%u] is 0x%02x, outside 0x21 .. 0x7e", i, (unsigned)(uint8_t)p->prefix[i]);
  if ((p->flags & KC_FASTQ_OUT_PACKED) && quals) return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: KC_FASTQ_OUT_PACKED and quals is not NULL");
  if (!(p->flags & KC_FASTQ_OUT_PACKED) && !quals && nreads)
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: quals is NULL for %llu reads without KC_FASTQ_OUT_PACKED", (unsigned long long)nreads);
  if (!order && n_order != nreads)
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: order is NULL and n_order %llu is not the %llu reads", (unsigned long long)n_order,
                (unsigned long long)nreads);
  if (nreads > 0xFFFFFFFFull || n_order > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_fastq_text: %llu reads and %llu records, read and record indices take 32 bits", (unsigned long long)nreads,
                (unsigned long long)n_order);
  if (!c) return KC_ERR_INVALID_ARG;
  if (nreads && !offsets) return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: offsets is NULL for %llu reads", (unsigned long long)nreads);
  if (on_device && (((uintptr_t)offsets & 7) || ((uintptr_t)ids & 7) || ((uintptr_t)order & 3)))
    return fail(KC_ERR_INVALID_ARG, "kc_fastq_text: device offsets and ids are 8-byte aligned, order 4-byte");
  return call_with_bufs(c, [&](CallBufs &b) {
    return rtext_run(c, b, bases, quals, offsets, nreads, order, n_order, ids, on_device, *p, first_byte, text, capacity, written, total);
  });
}
