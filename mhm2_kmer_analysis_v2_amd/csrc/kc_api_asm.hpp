// kc_api_asm.hpp -- kc_ctg_select, kc_fasta_text (kernels in kc_asm.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_shuffle.hpp; the check of the block is kc_align.hpp's, the radix passes are kc_sort.hpp's, the scan
// kc_api_call.hpp's.

static_assert(sizeof(kc_asm_params) == 32 && sizeof(kc_asm_stats) == 256 && sizeof(kc_fasta_params) == 64, "the header's layouts");
static_assert(KC_FASTA_MAX_PREFIX == ASM_MAX_PREFIX, "the header's limit is the kernels'");
namespace {
constexpr uint32_t asm_hdr_classes[] = KC_ASM_CLASSES, asm_classes[] = ASM_CLASS_LIST;
static_assert(sizeof(asm_hdr_classes) == sizeof(asm_classes) && sizeof(asm_classes) == ASM_NCLASSES * 4 && asm_hdr_classes[0] == asm_classes[0] &&
                  asm_hdr_classes[1] == asm_classes[1] && asm_hdr_classes[2] == asm_classes[2] && asm_hdr_classes[3] == asm_classes[3] &&
                  asm_hdr_classes[4] == asm_classes[4],
              "the header's classes are the kernels'");
}  // namespace

// what both calls ask of a block's arguments behind the context
static int asm_block_args(const char *who, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs) {
  if (!offsets || (nbytes && !seqs)) return KC_ERR_INVALID_ARG;
  if (nbytes >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "%s: a block of %llu bytes, positions take 31 bits (fewer than 2^31 bytes)", who, (unsigned long long)nbytes);
  if (n_ctgs > nbytes) {  // every contig has its separator
    return fail(KC_ERR_INVALID_ARG, "%s: %llu contigs in %llu bytes", who, (unsigned long long)n_ctgs, (unsigned long long)nbytes);
  }
  return KC_OK;
}

static int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll((unsigned long long)v) : 0; }

static int asm_select_run(kc_ctx *c, CallBufs &b, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, int on_device,
                          const kc_asm_params &prm, uint32_t *order, uint64_t *n_selected, kc_asm_stats *stats) {
  const bool dev = on_device != 0;
  const uint64_t tiles = (n_ctgs + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  const uint64_t max_sort_tiles = (n_ctgs + SORT_TILE - 1) / SORT_TILE;
  const uint64_t nspans = (nbytes + (1ull << ASM_SPAN_SHIFT) - 1) >> ASM_SPAN_SHIFT;
  AsmSelArgs a;
  memset(&a, 0, sizeof(a));
  uint64_t *d_ais, *kbuf[2] = {nullptr, nullptr}, *cnt = nullptr;
  uint32_t *ibuf[2] = {nullptr, nullptr}, *d_offs32, *tab;
  StagedIn<uint8_t> blk{seqs, dev, (size_t)nbytes, nbytes != 0};
  StagedIn<uint64_t> offs{offsets, dev, (size_t)(n_ctgs + 1) * 8};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(AS_COUNT);
    d_ais = m.take<uint64_t>(AIS_COUNT);
    zeroed = m.used;
    d_offs32 = m.take<uint32_t>(n_ctgs + 1);
    a.flag = m.take<uint64_t>(n_ctgs);
    a.fbase = m.take<uint64_t>(tiles);
    a.sel = m.take<uint32_t>(n_ctgs);
    a.by_len = m.take<uint32_t>(n_ctgs);
    kbuf[0] = m.take<uint64_t>(n_ctgs);
    kbuf[1] = m.take<uint64_t>(n_ctgs);
    ibuf[0] = m.take<uint32_t>(n_ctgs);
    ibuf[1] = m.take<uint32_t>(n_ctgs);
    cnt = m.take<uint64_t>(max_sort_tiles * SORT_DIGITS);
    tab = m.take<uint32_t>(nspans);
    blk.reserve(m);
    offs.reserve(m);
    return m.used;
  }));
  KCTRY(blk.upload(c));
  KCTRY(offs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(a.st + AS_SHORTEST, 0xFF, 8, c->stream));
  // ---- the check: nothing is stored through the caller's pointers before its verdict
  KCTRY(launch_timed(c, KT_ASM_CHECK, kc_align_check_kernel, blocks_for(std::max(nbytes, n_ctgs + 1)), dim3(256), 0, (const uint8_t *)blk.d, nbytes,
                     (const uint64_t *)offs.d, n_ctgs, d_offs32, d_ais));
  uint64_t ha[AIS_COUNT];
  KCTRY(read_back(c, ha, d_ais));
  if (ha[AIS_BAD_BASE]) return fail(KC_ERR_BAD_BASE, "kc_ctg_select: a byte outside ACGTN and '_' in the block");
  if (ha[AIS_BAD_OFFSETS] || ha[AIS_SEPARATORS] != n_ctgs)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_select: the offsets of %llu contigs do not match the block's %llu separators", (unsigned long long)n_ctgs,
                (unsigned long long)ha[AIS_SEPARATORS]);
  const dim3 tpb(ASM_TPB);
  uint64_t h[AS_COUNT];
  memset(h, 0, sizeof(h));
  a.offs = d_offs32;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.min_len = prm.min_len;
  a.keys = kbuf[0];
  int bits = 0;
  uint64_t nsel = 0;
  if (n_ctgs) {
    KCTRY(launch_timed(c, KT_ASM_LENS, kc_asm_lens_kernel, blocks_for(n_ctgs, ASM_TPB), tpb, 0, a));
    KCTRY(tiled_scan(c, KT_ASM_TILE_SCAN, KT_ASM_SCAN, a.flag, n_ctgs, a.fbase, a.st + AS_SCAN_SEL));
    KCTRY(launch_timed(c, KT_ASM_COMPACT, kc_asm_compact_kernel, blocks_for(n_ctgs, ASM_TPB), tpb, 0, a));
    KCTRY(read_back(c, h, a.st));
    nsel = h[AS_SELECTED];
  }
  if (nsel) {
    // ---- one stable sort of the permutation over the significant bits of longest - length: Nx needs it, flag or not
    bits = bit_length(h[AS_LONGEST] - h[AS_SHORTEST]);
    const uint64_t ntiles = (nsel + SORT_TILE - 1) / SORT_TILE, ncnt = ntiles * SORT_DIGITS;
    int cur = 0;
    const uint32_t *perm = nullptr;  // the identity until the first pass has run
    for (int shift = 0; shift < bits; shift += SORT_BITS) {
      const uint32_t mask = (1u << std::min(SORT_BITS, bits - shift)) - 1u;
      KCTRY(launch_timed(c, KT_ASM_SORT_HIST, kc_sort_hist_kernel<false>, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)nullptr, 1, 0,
                         perm, kbuf[cur], nsel, ntiles, shift, mask, cnt));
      KCTRY(launch_timed(c, KT_ASM_SORT_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{cnt}}, ncnt, a.st + AS_SORT_TOTAL));
      KCTRY(launch_timed(c, KT_ASM_SORT_SCATTER, kc_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)kbuf[cur], perm,
                         kbuf[cur ^ 1], ibuf[cur ^ 1], nsel, ntiles, shift, mask, (const uint64_t *)cnt));
      cur ^= 1;
      perm = ibuf[cur];
    }
    a.keys = kbuf[cur];
    a.perm = perm;
    a.nsel = nsel;
    // ---- the lengths in descending order, their sums, the two crossing points
    KCTRY(launch_timed(c, KT_ASM_SORTED, kc_asm_sorted_kernel, blocks_for(nsel, ASM_TPB), tpb, 0, a));
    KCTRY(tiled_scan(c, KT_ASM_LEN_TILE_SCAN, KT_ASM_LEN_SCAN, a.flag, nsel, a.fbase, a.st + AS_SCAN_BASES));
    KCTRY(launch_timed(c, KT_ASM_NX, kc_asm_nx_kernel, blocks_for(nsel, ASM_TPB), tpb, 0, a));
    // ---- the composition, by bytes
    if (h[AS_SEL_BASES]) {
      KCTRY(launch_timed(c, KT_ASM_SPANS, kc_asm_spans_kernel, blocks_for(nspans, ASM_TPB), tpb, 0, (const uint64_t *)offs.d, n_ctgs, (uint64_t)0, nspans,
                         tab));
      const uint64_t chunks = (nbytes + 15 + 15) / 16;  // a misaligned block's first chunk is partial
      KCTRY(launch_timed(c, KT_ASM_COMP, kc_asm_comp_kernel, blocks_for(chunks, ASM_TPB * ASM_COMP_SPANS), tpb, 0, (const uint8_t *)blk.d, nbytes,
                         (const uint64_t *)offs.d, n_ctgs, prm.min_len, (const uint32_t *)tab, a.st));
    }
    if (order)
      HIPCHK(hipMemcpyAsync(order, (prm.flags & KC_ASM_BY_LENGTH) ? a.by_len : a.sel, nsel * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            c->stream));
    KCTRY(read_back(c, h, a.st));
  }
  *n_selected = nsel;
  if (stats) {
    kc_asm_stats s;
    memset(&s, 0, sizeof(s));
    s.contigs = n_ctgs;
    s.bases = nbytes - n_ctgs;
    s.selected = nsel;
    s.sel_bases = h[AS_SEL_BASES];
    s.a = h[AS_A];
    s.c = h[AS_C];
    s.g = h[AS_G];
    s.t = h[AS_T];
    s.n = h[AS_N];
    s.n_runs = h[AS_N_RUNS];
    s.longest = nsel ? h[AS_LONGEST] : 0;
    s.shortest = nsel ? h[AS_SHORTEST] : 0;
    s.n50 = h[AS_N50];
    s.l50 = h[AS_L50];
    s.n90 = h[AS_N90];
    s.l90 = h[AS_L90];
    for (int j = 0; j < ASM_NCLASSES; j++) {
      s.ge_count[j] = h[AS_GE_COUNT + j];
      s.ge_bases[j] = h[AS_GE_BASES + j];
    }
    s.key_bits = (uint64_t)bits;
    *stats = s;
  }
  return KC_OK;
}

extern "C" int kc_ctg_select(kc_ctx *c, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, int on_device,
                             const kc_asm_params *p, uint32_t *order, uint64_t *n_selected, kc_asm_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_selected) return KC_ERR_INVALID_ARG;
  if (p->flags & ~KC_ASM_BY_LENGTH) return fail(KC_ERR_INVALID_ARG, "kc_ctg_select: unknown flags 0x%x", p->flags & ~KC_ASM_BY_LENGTH);
  for (int i = 0; i < 6; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_ctg_select: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (!c) return KC_ERR_INVALID_ARG;
  KCTRY(asm_block_args("kc_ctg_select", seqs, nbytes, offsets, n_ctgs));
  if (on_device && (((uintptr_t)offsets & 7) || ((uintptr_t)order & 3)))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_select: device offsets are 8-byte aligned, order 4-byte");
  return call_with_bufs(c, [&](CallBufs &b) { return asm_select_run(c, b, seqs, nbytes, offsets, n_ctgs, on_device, *p, order, n_selected, stats); });
}

static int asm_text_run(kc_ctx *c, CallBufs &b, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, const uint32_t *order,
                        uint64_t n_order, int on_device, const kc_fasta_params &prm, uint64_t first_byte, uint8_t *text, uint64_t capacity,
                        uint64_t *written, uint64_t *total) {
  const bool dev = on_device != 0;
  const uint64_t tiles = (n_order + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  AsmTextArgs a;
  memset(&a, 0, sizeof(a));
  uint8_t *d_prefix;
  StagedIn<uint8_t> blk{seqs, dev, (size_t)nbytes, nbytes != 0};
  StagedIn<uint64_t> offs{offsets, dev, (size_t)(n_ctgs + 1) * 8};
  StagedIn<uint32_t> ord{order, dev, (size_t)n_order * 4, order != nullptr};
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(AT_COUNT);
    d_prefix = m.take<uint8_t>(ASM_MAX_PREFIX);
    a.rs = m.take<uint64_t>(n_order + 1);
    a.rbase = m.take<uint64_t>(tiles);
    blk.reserve(m);
    offs.reserve(m);
    ord.reserve(m, order != nullptr);
    return m.used;
  }));
  KCTRY(blk.upload(c));
  KCTRY(offs.upload(c));
  KCTRY(ord.upload(c));
  HIPCHK(hipMemcpyAsync(d_prefix, prm.prefix, ASM_MAX_PREFIX, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(a.st, 0, AT_COUNT * 8, c->stream));
  HIPCHK(hipMemsetAsync(a.st + AT_BAD_ORDER, 0xFF, 8, c->stream));
  a.seqs = blk.d;
  a.nbytes = nbytes;
  a.offs = offs.d;
  a.n_ctgs = n_ctgs;
  a.order = order ? ord.d : nullptr;
  a.n_order = n_order;
  a.prefix = d_prefix;
  a.prefix_len = prm.prefix_len;
  a.lw = prm.line_width ? prm.line_width : 0xFFFFFFFEu;
  a.lwp1 = a.lw + 1u;
  a.first_byte = first_byte;
  const dim3 tpb(ASM_TPB);
  // ---- the checks: their verdict is read before a size is formed from an offset or an order entry
  KCTRY(launch_timed(c, KT_ASM_TEXT_CHECK, kc_asm_text_check_kernel, blocks_for(std::max(n_ctgs + 1, n_order), ASM_TPB), tpb, 0, a));
  uint64_t h[AT_COUNT];
  KCTRY(read_back(c, h, a.st));
  if (h[AT_BAD_OFFSETS])
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: the offsets of %llu contigs do not match the block's separators", (unsigned long long)n_ctgs);
  if (h[AT_BAD_ORDER] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: order[%llu] names no contig (%llu contigs)", (unsigned long long)h[AT_BAD_ORDER],
                (unsigned long long)n_ctgs);
  // ---- the records' starts and the total
  uint64_t all = 0;
  if (n_order) {
    KCTRY(launch_timed(c, KT_ASM_SIZES, kc_asm_sizes_kernel, blocks_for(n_order, ASM_TPB), tpb, 0, a));
    KCTRY(tiled_scan(c, KT_ASM_TEXT_TILE_SCAN, KT_ASM_TEXT_SCAN, a.rs, n_order, a.rbase, a.st + AT_TOTAL));
    KCTRY(launch_timed(c, KT_ASM_STARTS, kc_asm_starts_kernel, blocks_for(n_order + 1, ASM_TPB), tpb, 0, a));
    KCTRY(read_back(c, &all, a.st + AT_TOTAL, 1));
  }
  if (first_byte > all)
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: first_byte %llu is behind the text's %llu bytes", (unsigned long long)first_byte,
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
    KCTRY(launch_timed(c, KT_ASM_TEXT_SPANS, kc_asm_spans_kernel, blocks_for(nspans, ASM_TPB), tpb, 0, (const uint64_t *)a.rs, n_order, first_byte, nspans,
                       tab));
    const uint64_t chunks = (n + 15 + 15) / 16;  // a misaligned array's first chunk is partial
    KCTRY(launch_timed(c, KT_ASM_WRITE, kc_asm_write_kernel, blocks_for(chunks, ASM_TPB), tpb, 0, a));
    if (!dev) HIPCHK(hipMemcpyAsync(text, d_text, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  *written = n;
  *total = all;
  return KC_OK;
}

extern "C" int kc_fasta_text(kc_ctx *c, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, const uint32_t *order,
                             uint64_t n_order, int on_device, const kc_fasta_params *p, uint64_t first_byte, uint8_t *text, uint64_t capacity,
                             uint64_t *written, uint64_t *total) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p) return KC_ERR_INVALID_ARG;
  if (p->line_width > 65535) return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: line_width %u over 65535", p->line_width);
  if (p->prefix_len > KC_FASTA_MAX_PREFIX)
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: prefix_len %u over %d", p->prefix_len, KC_FASTA_MAX_PREFIX);
  for (uint32_t i = 0; i < p->prefix_len; i++)
    if ((uint8_t)p->prefix[i] < 0x21 || (uint8_t)p->prefix[i] > 0x7E)
      return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: prefix[%u] is 0x%02x, outside 0x21 .. 0x7e", i, (unsigned)(uint8_t)p->prefix[i]);
  if (p->flags) return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: unknown flags 0x%x", p->flags);
  if (p->reserved0 || p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3])
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: reserved words %u %u %u %u %u, not zero", p->reserved0, p->reserved[0], p->reserved[1],
                p->reserved[2], p->reserved[3]);
  if (!written || !total) return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: %s is NULL", written ? "total" : "written");
  if (!order && n_order != n_ctgs)
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: order is NULL and n_order %llu is not the %llu contigs", (unsigned long long)n_order,
                (unsigned long long)n_ctgs);
  if (!c) return KC_ERR_INVALID_ARG;
  KCTRY(asm_block_args("kc_fasta_text", seqs, nbytes, offsets, n_ctgs));
  if (on_device && (((uintptr_t)offsets & 7) || ((uintptr_t)order & 3)))
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_text: device offsets are 8-byte aligned, order 4-byte");
  if (n_order > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_fasta_text: %llu records, the window's table holds 32-bit record indices", (unsigned long long)n_order);
  return call_with_bufs(c, [&](CallBufs &b) {
    return asm_text_run(c, b, seqs, nbytes, offsets, n_ctgs, order, n_order, on_device, *p, first_byte, text, capacity, written, total);
  });
}
