// kc_api_fasta_in.hpp -- kc_fasta_to_block (kernels in kc_fasta_in.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_asm.hpp; the line index is kc_fastq.hpp's, the scans kc_api_call.hpp's.

static_assert(sizeof(kc_fasta_in_params) == 32 && sizeof(kc_fasta_in_stats) == 128 && sizeof(kc_fasta_rec) == sizeof(FaRec), "the header's layouts");
static_assert(KC_FASTA_HDR_SCAN == FA_HDR_SCAN && KC_FASTA_HAS_ID == FA_HAS_ID && KC_FASTA_HAS_DEPTH == FA_HAS_DEPTH && KC_FASTA_LOWERED == FA_LOWERED &&
                  KC_FASTA_RECODED == FA_RECODED,
              "the header's constants are the kernels'");
static_assert(offsetof(kc_fasta_rec, hdr_len) == offsetof(FaRec, hdr_len) && offsetof(kc_fasta_rec, id) == offsetof(FaRec, id) &&
                  offsetof(kc_fasta_rec, flags) == offsetof(FaRec, flags),
              "the header's record is the kernels'");

static int fasta_in_run(kc_ctx *c, CallBufs &b, const uint8_t *text, uint64_t len, int on_device, const kc_fasta_in_params &prm, uint8_t *seqs,
                        uint64_t seqs_capacity, uint64_t *offsets, uint64_t ctgs_capacity, uint16_t *depths, kc_fasta_rec *recs, uint64_t *n_ctgs,
                        uint64_t *nbytes, uint64_t *consumed, kc_fasta_in_stats *stats) {
  const bool dev = on_device != 0, partial = (prm.flags & KC_FASTA_PARTIAL) != 0;
  const dim3 tpb(FA_TPB);
  // ---- the text, and the FASTQ parser's line index over it
  FqFile f;
  memset(&f, 0, sizeof(f));
  StagedIn<uint8_t> txt{text, dev, (size_t)len, len != 0};
  uint64_t *st;
  f.len = len;
  f.ntiles = (15 + len + FQ_TILE - 1) / FQ_TILE;  // at most: the staged text's alignment is not known yet
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    st = m.take<uint64_t>(FAS_COUNT);
    f.tile = m.take<uint64_t>(f.ntiles);
    txt.reserve(m);
    return m.used;
  }));
  KCTRY(txt.upload(c));
  f.text = txt.d;
  f.head = len ? (uint64_t)((uintptr_t)f.text & 15u) : 0;
  f.ntiles = (f.head + len + FQ_TILE - 1) / FQ_TILE;
  HIPCHK(hipMemsetAsync(st, 0, FAS_COUNT * 8, c->stream));
  HIPCHK(hipMemsetAsync(st + FAS_KEY, 0xFF, 8, c->stream));
  uint8_t last = '\n';
  if (f.ntiles) KCTRY(launch_timed(c, KT_FA_COUNT, kc_fq_count_kernel, fq_grid(f.ntiles), dim3(FQ_TPB), 0, f));
  KCTRY(launch_timed(c, KT_FA_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{f.tile}}, f.ntiles, st + FAS_NNL));
  if (len) HIPCHK(hipMemcpyAsync(&last, f.text + len - 1, 1, hipMemcpyDeviceToHost, c->stream));
  uint64_t h[FAS_COUNT];
  KCTRY(read_back(c, h, st));
  f.nnl = h[FAS_NNL];
  KCTRY(b.alloc(&f.ends, f.nnl * 8));
  if (f.ntiles && f.nnl) KCTRY(launch_timed(c, KT_FA_INDEX, kc_fq_index_kernel, fq_grid(f.ntiles), dim3(FQ_TPB), 0, f));
  // ---- the lines
  FaArgs a;
  memset(&a, 0, sizeof(a));
  a.text = f.text;
  a.len = len;
  a.ends = f.ends;
  a.nnl = f.nnl;
  a.nl = f.nnl + (len && last != '\n' ? 1 : 0);
  a.st = st;
  a.strict = (prm.flags & KC_FASTA_STRICT) ? 1u : 0u;
  a.default_depth = prm.default_depth;
  const uint64_t tiles = (a.nl + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.v = m.take<uint64_t>(a.nl + 1);
    a.h = m.take<uint64_t>(a.nl + 1);
    a.e = m.take<uint64_t>(a.nl + 1);
    a.vbase = m.take<uint64_t>(tiles);
    a.hbase = m.take<uint64_t>(tiles);
    a.ebase = m.take<uint64_t>(tiles);
    return m.used;
  }));
  if (a.nl) KCTRY(launch_timed(c, KT_FA_LINES, kc_fa_lines_kernel, blocks_for(a.nl, FA_TPB), tpb, 0, a, partial ? 1 : 0));
  uint64_t used = len;
  if (partial) {  // the text ends in front of its last header: the lines in front of that are whole, each with its '\n'
    uint64_t hl = 0;
    KCTRY(read_back(c, &hl, st + FAS_LAST, 1));
    used = 0;
    if (hl > 1) {
      KCTRY(read_back(c, &used, a.ends + (hl - 2), 1));
      used++;
    }
    a.len = used;
    a.nl = a.nnl = hl ? hl - 1 : 0;
  }
  // ---- block bytes, headers and non-empty sequence lines in front of every line
  memset(h, 0, sizeof(h));
  if (a.nl) {
    KCTRY(tiled_scan(c, KT_FA_TILE_SCAN, KT_FA_LINE_SCAN, a.v, a.nl, a.vbase, st + FAS_NBYTES));
    KCTRY(tiled_scan(c, KT_FA_TILE_SCAN, KT_FA_LINE_SCAN, a.h, a.nl, a.hbase, st + FAS_HEADERS));
    KCTRY(tiled_scan(c, KT_FA_TILE_SCAN, KT_FA_LINE_SCAN, a.e, a.nl, a.ebase, st + FAS_SEQ_LINES));
    KCTRY(read_back(c, h, st));
  }
  a.nbytes = h[FAS_NBYTES];
  a.n_ctgs = h[FAS_HEADERS];
  const uint64_t text_spans = (a.len + (1ull << FA_SPAN_SHIFT) - 1) >> FA_SPAN_SHIFT, block_spans = (a.nbytes + (1ull << FA_SPAN_SHIFT) - 1) >> FA_SPAN_SHIFT;
  uint64_t *text_tab, *block_tab;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.hline = m.take<uint64_t>(a.n_ctgs + 1);
    a.roff = m.take<uint64_t>(a.n_ctgs + 1);
    a.rflags = m.take<uint32_t>(a.n_ctgs);
    a.recs = m.take<FaRec>(a.n_ctgs);
    text_tab = m.take<uint64_t>(text_spans);
    block_tab = m.take<uint64_t>(block_spans);
    return m.used;
  }));
  if (a.n_ctgs) HIPCHK(hipMemsetAsync(a.rflags, 0, a.n_ctgs * 4, c->stream));
  KCTRY(launch_timed(c, KT_FA_STARTS, kc_fa_starts_kernel, blocks_for(a.nl + 1, FA_TPB), tpb, 0, a));
  // ---- the validation: its verdict is read before anything is stored through the caller's pointers
  if (a.nl && a.len) {
    a.tab = text_tab;
    KCTRY(launch_timed(c, KT_FA_SPANS, kc_fa_spans_kernel, blocks_for(text_spans, FA_TPB), tpb, 0, a, 0, text_spans, text_tab));
    const uint64_t chunks = (a.len + 15 + 15) / 16;  // a misaligned text's first chunk is partial
    KCTRY(launch_timed(c, KT_FA_CHECK, kc_fa_check_kernel, blocks_for(chunks, FA_TPB), tpb, 0, a));
    KCTRY(launch_timed(c, KT_FA_DETAIL, kc_fa_detail_kernel, dim3(1), dim3(64), 0, a));
  }
  if (a.n_ctgs) KCTRY(launch_timed(c, KT_FA_RECS, kc_fa_recs_kernel, blocks_for(a.n_ctgs, FA_TPB), tpb, 0, a));
  KCTRY(read_back(c, h, st));
  if (h[FAS_KEY] != ~0ull) {
    if (h[FAS_KEY] & 1)
      return fail(KC_ERR_BAD_BASE, "fasta: line %llu column %llu: byte 0x%02x is not a base", (unsigned long long)h[FAS_ERR_LINE],
                  (unsigned long long)h[FAS_ERR_COL], (unsigned)h[FAS_ERR_BYTE]);
    return fail(KC_ERR_INVALID_ARG, "fasta: line %llu: sequence before the first header", (unsigned long long)h[FAS_ERR_LINE]);
  }
  // ---- the totals
  *n_ctgs = a.n_ctgs;
  *nbytes = a.nbytes;
  if (consumed) *consumed = used;
  if (stats) {
    kc_fasta_in_stats s;
    memset(&s, 0, sizeof(s));
    s.lines = a.nl;
    s.empty_lines = a.nl - a.n_ctgs - h[FAS_SEQ_LINES];
    s.records = a.n_ctgs;
    s.empty_records = h[FAS_EMPTY_RECS];
    s.bases = a.nbytes - a.n_ctgs;
    s.lowered = h[FAS_LOWERED];
    s.recoded = h[FAS_RECODED];
    s.longest = h[FAS_LONGEST];
    s.with_id = h[FAS_WITH_ID];
    s.with_depth = h[FAS_WITH_DEPTH];
    *stats = s;
  }
  if (a.nbytes >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_fasta_to_block: a block of %llu bytes, positions take 31 bits (fewer than 2^31 bytes)",
                (unsigned long long)a.nbytes);
  if (!seqs || !offsets) return KC_OK;  // a size query
  if (a.nbytes > seqs_capacity || a.n_ctgs > ctgs_capacity)
    return fail(KC_ERR_CAPACITY, "kc_fasta_to_block: %llu contigs in %llu bytes do not fit the arrays", (unsigned long long)a.n_ctgs,
                (unsigned long long)a.nbytes);
  // ---- the block
  StagedOut<uint8_t> out{seqs, dev, (size_t)a.nbytes};
  StagedOut<uint16_t> dep{depths, dev, (size_t)a.nbytes * 2};
  if (!dev)
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      out.reserve(m);
      dep.reserve(m);
      return m.used;
    }));
  else {
    out.d = seqs;
    dep.d = depths;
  }
  const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (a.nbytes) {
    a.seqs = out.d;
    a.depths = dep.d;
    a.tab = block_tab;
    KCTRY(launch_timed(c, KT_FA_BLOCK_SPANS, kc_fa_spans_kernel, blocks_for(block_spans, FA_TPB), tpb, 0, a, 1, block_spans, block_tab));
    const uint64_t chunks = (a.nbytes + 15 + 15) / 16;  // a misaligned array's first chunk is partial
    KCTRY(launch_timed(c, KT_FA_WRITE, kc_fa_write_kernel, blocks_for(chunks, FA_TPB), tpb, 0, a));
    KCTRY(out.download(c));
    KCTRY(dep.download(c));
  }
  HIPCHK(hipMemcpyAsync(offsets, a.roff, (a.n_ctgs + 1) * 8, back, c->stream));
  if (recs && a.n_ctgs) HIPCHK(hipMemcpyAsync(recs, a.recs, a.n_ctgs * sizeof(FaRec), back, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

extern "C" int kc_fasta_to_block(kc_ctx *c, const uint8_t *text, uint64_t len, int on_device, const kc_fasta_in_params *p, uint8_t *seqs,
                                 uint64_t seqs_capacity, uint64_t *offsets, uint64_t ctgs_capacity, uint16_t *depths, kc_fasta_rec *recs, uint64_t *n_ctgs,
                                 uint64_t *nbytes, uint64_t *consumed, kc_fasta_in_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_ctgs || !nbytes) return fail(KC_ERR_INVALID_ARG, "kc_fasta_to_block: %s is NULL", !p ? "params" : !n_ctgs ? "n_ctgs" : "nbytes");
  if (p->flags & ~(KC_FASTA_PARTIAL | KC_FASTA_STRICT))
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_to_block: unknown flags 0x%x", p->flags & ~(KC_FASTA_PARTIAL | KC_FASTA_STRICT));
  if (p->default_depth > 65535) return fail(KC_ERR_INVALID_ARG, "kc_fasta_to_block: default_depth %u over 65535", p->default_depth);
  for (int i = 0; i < 6; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_fasta_to_block: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (!c || (len && !text)) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)offsets & 7) || ((uintptr_t)recs & 7) || ((uintptr_t)depths & 1)))
    return fail(KC_ERR_INVALID_ARG, "kc_fasta_to_block: device offsets and recs are 8-byte aligned, depths 2-byte");
  return call_with_bufs(c, [&](CallBufs &b) {
    return fasta_in_run(c, b, text, len, on_device, *p, seqs, seqs_capacity, offsets, ctgs_capacity, depths, recs, n_ctgs, nbytes, consumed, stats);
  });
}
