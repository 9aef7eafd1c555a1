// kc_api_depth.hpp -- kc_ctg_index_info, kc_aln_depths, kc_pair_inserts (kernels in kc_depth.hpp).  Part of kc_api.hip's
// translation unit, behind kc_api_gap.hpp.

static_assert(sizeof(kc_ctg_depth) == 32, "a record is two 16-byte stores");
static_assert(sizeof(kc_pair_rec) == 16, "a record is one 16-byte store");
static_assert(sizeof(kc_depth_stats) == 72 && sizeof(kc_insert_stats) == 88, "nine and eleven counters");
static_assert(KC_DEPTH_MAX_EDGE == DEPTH_MAX_EDGE && KC_DEPTH_BEST_ONLY == DEPTH_BEST_ONLY && KC_DEPTH_PER_CONTIG == DEPTH_PER_CONTIG,
              "the header's constants are the kernels'");
static_assert(KC_INSERT_MAX == PAIR_INSERT_MAX && KC_PAIR_NONE == PAIR_NONE && KC_PAIR_ONE == PAIR_ONE && KC_PAIR_DIFF_CTG == PAIR_DIFF_CTG &&
                  KC_PAIR_SAME_ORIENT == PAIR_SAME_ORIENT && KC_PAIR_EVERTED == PAIR_EVERTED && KC_PAIR_TOO_LONG == PAIR_TOO_LONG &&
                  KC_PAIR_PROPER == PAIR_PROPER,
              "the header's classes");

extern "C" int kc_ctg_index_info(kc_ctx *c, uint64_t *nbytes, uint64_t *n_ctgs) {
  if (!c) return KC_ERR_INVALID_ARG;
  if (!c->ai_ready) return no_ctg_index("kc_ctg_index_info");
  if (nbytes) *nbytes = c->ai_nbytes;
  if (n_ctgs) *n_ctgs = c->ai.n_ctgs;
  return KC_OK;
}

static int depth_run(kc_ctx *c, CallBufs &b, const kc_gap_aln *alns, uint64_t n_alns, uint64_t nreads, int on_device, uint32_t min_score,
                     uint32_t min_len, uint32_t edge_clip, uint32_t flags, uint16_t *depths, kc_ctg_depth *ctgs, kc_depth_stats *stats) {
  const uint64_t nbytes = c->ai_nbytes, n_ctgs = c->ai.n_ctgs;
  const uint64_t tiles = (nbytes + DEPTH_TILE - 1) / DEPTH_TILE;
  const bool best_only = (flags & DEPTH_BEST_ONLY) != 0, per_contig = (flags & DEPTH_PER_CONTIG) != 0;
  const bool dev = on_device != 0;
  DepthArgs a;
  memset(&a, 0, sizeof(a));
  StagedIn<uint4> in{alns, dev, n_alns * sizeof(kc_gap_aln)};
  StagedOut<uint16_t> out_depths{depths, dev, nbytes * 2};
  StagedOut<uint4> out_ctgs{ctgs, dev, n_ctgs * sizeof(kc_ctg_depth)};
  size_t zeroed = 0;  // the front of the scratch is counters and sums: one memset
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(DPS_COUNT);
    a.diff = m.take<uint32_t>(tiles * DEPTH_TILE);
    a.tile_sums = m.take<uint64_t>(tiles);
    a.csum = m.take<uint64_t>(n_ctgs);
    a.ccov = m.take<uint32_t>(n_ctgs);
    a.cmax = m.take<uint32_t>(n_ctgs);
    a.calns = m.take<uint32_t>(n_ctgs);
    a.best = m.take<uint64_t>(best_only ? nreads : 0);
    zeroed = m.used;
    a.cmin = m.take<uint32_t>(n_ctgs);
    a.cmean = m.take<uint32_t>(n_ctgs);
    in.reserve(m);
    out_depths.reserve(m);
    out_ctgs.reserve(m);
    return m.used;
  }));
  KCTRY(in.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(a.st + DPS_BAD, 0xFF, 8, c->stream));
  if (n_ctgs) HIPCHK(hipMemsetAsync(a.cmin, 0xFF, n_ctgs * 4, c->stream));
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.nbytes = (uint32_t)nbytes;
  a.alns = in.d;
  a.n_alns = n_alns;
  a.nreads = nreads;
  a.min_score = min_score;
  a.min_len = min_len;
  a.edge_clip = edge_clip;
  a.flags = flags;
  a.depths = out_depths.d;
  a.ctgs = out_ctgs.d;
  KCTRY(depth_check(c, a, KT_DEPTH_CHECK, best_only ? 1 : 0, "kc_aln_depths"));
  if (n_alns) {
    if (best_only) KCTRY(launch_timed(c, KT_DEPTH_BEST, kc_depth_best_kernel, blocks_for(n_alns), dim3(256), 0, a));
    KCTRY(launch_timed(c, KT_DEPTH_MARK, kc_depth_mark_kernel, blocks_for(n_alns), dim3(256), 0, a));
  }
  if (tiles) {
    const dim3 grid((unsigned)tiles), tpb(DEPTH_TPB);
    KCTRY(launch_timed(c, KT_DEPTH_TILE_SUMS, kc_depth_tile_sums_kernel, grid, tpb, 0, a));
    KCTRY(launch_timed(c, KT_DEPTH_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.tile_sums}}, tiles, a.st + DPS_TOTAL));
    KCTRY(launch_timed(c, KT_DEPTH_RESCAN, kc_depth_rescan_kernel, grid, tpb, 0, a, (depths && !per_contig) ? 1 : 0));
    if (ctgs || (depths && per_contig)) KCTRY(launch_timed(c, KT_DEPTH_CTG, kc_depth_ctg_kernel, blocks_for(n_ctgs), dim3(256), 0, a));
    if (depths && per_contig) KCTRY(launch_timed(c, KT_DEPTH_FILL, kc_depth_fill_kernel, grid, tpb, 0, a));
  }
  KCTRY(out_depths.download(c));
  KCTRY(out_ctgs.download(c));
  uint64_t h[DPS_COUNT];
  KCTRY(read_back(c, h, a.st));
  if (stats) {
    stats->records = n_alns;
    stats->none = h[DPS_NONE];
    stats->filtered = h[DPS_FILTERED];
    stats->not_best = h[DPS_NOT_BEST];
    stats->clipped_away = h[DPS_CLIPPED];
    stats->used = h[DPS_USED];
    stats->bases_covered = h[DPS_COVERED];
    stats->depth_sum = h[DPS_DEPTH_SUM];
    stats->saturated = h[DPS_SATURATED];
  }
  return KC_OK;
}

extern "C" int kc_aln_depths(kc_ctx *c, const kc_gap_aln *alns, uint64_t n_alns, uint64_t nreads, int on_device, uint32_t min_score,
                             uint32_t min_len, uint32_t edge_clip, uint32_t flags, uint16_t *depths, kc_ctg_depth *ctgs, kc_depth_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (edge_clip > KC_DEPTH_MAX_EDGE || (flags & ~(KC_DEPTH_BEST_ONLY | KC_DEPTH_PER_CONTIG)))
    return fail(KC_ERR_INVALID_ARG, "kc_aln_depths: edge_clip %u over %d or unknown flags 0x%x", edge_clip, KC_DEPTH_MAX_EDGE, flags);
  if (!c || (n_alns && !alns)) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)ctgs) & 15)) return misaligned_records("kc_aln_depths");
  if (on_device && ((uintptr_t)depths & 1)) return fail(KC_ERR_INVALID_ARG, "kc_aln_depths: a device depth array is 2-byte aligned");
  if (!c->ai_ready) return no_ctg_index("kc_aln_depths");
  if (n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_aln_depths: %llu records, a depth and a best record's index hold 32 bits", (unsigned long long)n_alns);
  return call_with_bufs(c, [&](CallBufs &b) {
    return depth_run(c, b, alns, n_alns, nreads, on_device, min_score, min_len, edge_clip, flags, depths, ctgs, stats);
  });
}

static int pair_run(kc_ctx *c, CallBufs &b, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, int on_device,
                    uint32_t min_score, uint32_t min_len, uint32_t max_insert, uint64_t *hist, kc_pair_rec *pairs, kc_insert_stats *stats) {
  const uint64_t npairs = nreads / 2, nbins = (uint64_t)max_insert + 1;
  const bool dev = on_device != 0;
  DepthArgs a;
  memset(&a, 0, sizeof(a));
  uint64_t *d_als, *d_pst;
  StagedIn<uint64_t> offs = staged_offsets(offsets, nreads, dev);
  StagedIn<uint4> in{alns, dev, n_alns * sizeof(kc_gap_aln)};
  StagedOut<uint64_t> out_hist{hist, dev, nbins * 8};
  StagedOut<uint4> out_pairs{pairs, dev, npairs * sizeof(kc_pair_rec)};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(DPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    d_pst = m.take<uint64_t>(PRS_COUNT);
    a.best = m.take<uint64_t>(nreads);
    zeroed = m.used;
    offs.reserve(m);
    in.reserve(m);
    out_hist.reserve(m);
    out_pairs.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(in.upload(c));
  uint64_t *const d_hist = out_hist.d;
  uint4 *const d_pairs = out_pairs.d;
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(a.st + DPS_BAD, 0xFF, 8, c->stream));
  KCTRY(check_read_lengths(c, KT_PAIR_LENGTHS, "kc_pair_inserts", offs.d, nreads, d_als));
  a.min_score = min_score;
  a.min_len = min_len;
  KCTRY(check_read_records(c, a, KT_PAIR_CHECK, "kc_pair_inserts", in.d, n_alns, offs.d, nreads));
  if (n_alns) KCTRY(launch_timed(c, KT_PAIR_BEST, kc_depth_best_kernel, blocks_for(n_alns), dim3(256), 0, a));
  if (hist) HIPCHK(hipMemsetAsync(d_hist, 0, nbins * 8, c->stream));
  if (npairs) {
    // enough workgroups to fill the device; each brings its bins once
    const dim3 grid((unsigned)std::min<uint64_t>((npairs + PAIR_TPB - 1) / PAIR_TPB, 2048));
    if (nbins <= PAIR_LDS_BINS)
      KCTRY(launch_timed(c, KT_PAIR_CLASSIFY_LDS, kc_pair_classify_kernel<true>, grid, dim3(PAIR_TPB), 0, a, max_insert, d_hist, d_pairs, d_pst));
    else
      KCTRY(launch_timed(c, KT_PAIR_CLASSIFY, kc_pair_classify_kernel<false>, grid, dim3(PAIR_TPB), 0, a, max_insert, d_hist, d_pairs, d_pst));
  }
  KCTRY(out_hist.download(c));
  KCTRY(out_pairs.download(c));
  uint64_t h[PRS_COUNT];
  KCTRY(read_back(c, h, d_pst));
  if (stats) {
    stats->pairs = npairs;
    for (int k = 0; k < PAIR_CLASSES; k++) stats->cls[k] = h[PRS_CLS + k];
    stats->insert_sum = h[PRS_INSERT_SUM];
    stats->insert_sq_sum = h[PRS_INSERT_SQ];
    stats->reads_with_best = h[PRS_WITH_BEST];
  }
  return KC_OK;
}

extern "C" int kc_pair_inserts(kc_ctx *c, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, int on_device,
                               uint32_t min_score, uint32_t min_len, uint32_t max_insert, uint64_t *hist, kc_pair_rec *pairs,
                               kc_insert_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (max_insert < 1 || max_insert > KC_INSERT_MAX)
    return fail(KC_ERR_INVALID_ARG, "kc_pair_inserts: max_insert %u outside 1 .. %d", max_insert, KC_INSERT_MAX);
  if (nreads & 1)
    return fail(KC_ERR_INVALID_ARG, "kc_pair_inserts: %llu reads are no pairs (reads 2p and 2p + 1 are mates)", (unsigned long long)nreads);
  if (!c || (nreads && !offsets) || (n_alns && !alns) || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs) & 15)) return misaligned_records("kc_pair_inserts");
  if (on_device && (((uintptr_t)offsets | (uintptr_t)hist) & 7))
    return fail(KC_ERR_INVALID_ARG, "kc_pair_inserts: device offsets and bins are 8-byte aligned");
  if (!c->ai_ready) return no_ctg_index("kc_pair_inserts");
  if (n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_pair_inserts: %llu records, a best record's index holds 32 bits", (unsigned long long)n_alns);
  return call_with_bufs(c, [&](CallBufs &b) {
    return pair_run(c, b, offsets, nreads, alns, n_alns, on_device, min_score, min_len, max_insert, hist, pairs, stats);
  });
}
