// kc_api_gap.hpp -- kc_align_gapped (kernels in kc_gap.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_align.hpp, whose AlignBufs and length check it uses.

static_assert(sizeof(kc_gap_aln) == 32, "a record is two 16-byte stores");
static_assert(sizeof(kc_gap_stats) == 48, "six counters");
static_assert(KC_GAP_MAX_PAD == GAP_MAX_PAD && KC_GAP_ALWAYS_DP == GAP_ALWAYS_DP, "the header's constants are the kernels'");
static_assert(KC_GAP_EXACT == GAP_KIND_EXACT && KC_GAP_DP == GAP_KIND_DP && KC_GAP_NONE == GAP_KIND_NONE, "the header's kinds");

static int gap_run(kc_ctx *c, AlignBufs &b, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, const kc_read_aln *alns,
                   uint64_t n_alns, int on_device, uint32_t pad, const kc_aln_scores *sc, uint32_t flags, kc_gap_aln *out,
                   kc_gap_stats *stats) {
  uint64_t *d_st, *d_als, *d_list, *d_offs = nullptr;
  uint4 *d_in = nullptr, *d_out = nullptr;
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    d_st = m.take<uint64_t>(GPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    d_list = m.take<uint64_t>(n_alns);
    if (!on_device) {
      d_offs = m.take<uint64_t>(nreads + 1);
      d_in = m.take<uint4>(2 * n_alns);
      d_out = m.take<uint4>(2 * n_alns);
    }
    return m.used;
  };
  HIPCHK(hipMalloc((void **)&b.a, layout(nullptr)));
  layout(b.a);
  if (!on_device) {
    if (nreads) HIPCHK(hipMemcpyAsync(d_offs, offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_in, alns, n_alns * sizeof(kc_read_aln), hipMemcpyHostToDevice, c->stream));
  } else {
    d_offs = const_cast<uint64_t *>(offsets);
    d_in = (uint4 *)const_cast<kc_read_aln *>(alns);
    d_out = (uint4 *)out;
  }
  HIPCHK(hipMemsetAsync(d_st, 0, GPS_COUNT * 8, c->stream));
  HIPCHK(hipMemsetAsync(d_st + GPS_BAD, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d_als, 0, ALS_COUNT * 8, c->stream));
  HIPCHK(hipMemsetAsync(d_als + ALS_BAD_READ, 0xFF, 8, c->stream));
  uint64_t h_als[ALS_COUNT], last = 0;
  h_als[ALS_BAD_READ] = ~0ull;
  h_als[ALS_MAX_LEN] = 0;
  if (nreads) {
    KCTRY(launch_timed(c, KT_GAP_LENGTHS, kc_align_lengths_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, (const uint64_t *)d_offs,
                       nreads, d_als));
    HIPCHK(hipMemcpyAsync(h_als, d_als, sizeof(h_als), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&last, d_offs + nreads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (h_als[ALS_BAD_READ] != ~0ull) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_align_gapped: read %llu is longer than %d bases, or its offsets decrease",
             (unsigned long long)h_als[ALS_BAD_READ], KC_ALIGN_MAX_READ_LEN);
    return KC_ERR_INVALID_ARG;
  }
  if (last && !bases) return KC_ERR_INVALID_ARG;
  const uint8_t *d_bases = bases;
  if (!on_device && last) {  // lengths are checked: the reads are the first `last` bytes
    HIPCHK(hipMalloc((void **)&b.b, last));
    HIPCHK(hipMemcpyAsync(b.b, bases, last, hipMemcpyHostToDevice, c->stream));
    d_bases = b.b;
  }
  GapArgs a;
  a.ix = c->ai;
  a.bases = d_bases;
  a.offsets = d_offs;
  a.nreads = nreads;
  a.alns = d_in;
  a.n_alns = n_alns;
  a.out = d_out;
  a.pad = pad;
  a.flags = flags;
  a.match = (int)sc->match;
  a.mismatch = (int)sc->mismatch;
  a.gap_open = (int)sc->gap_open;
  a.gap_ext = (int)sc->gap_ext;
  a.amb = (int)sc->ambiguity;
  a.list = d_list;
  a.st = d_st;
  KCTRY(launch_timed(c, KT_GAP_CHECK, kc_gap_check_kernel, dim3((unsigned)((n_alns + 255) / 256)), dim3(256), 0, a));
  uint64_t h[GPS_COUNT];
  HIPCHK(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (h[GPS_BAD] != ~0ull) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_align_gapped: record %llu is not one kc_align_reads emits for these reads and this index",
             (unsigned long long)h[GPS_BAD]);
    return KC_ERR_INVALID_ARG;
  }
  // a wave per record, or a few records a wave once every compute unit is full
  auto waves_grid = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + GAP_WAVES - 1) / GAP_WAVES, 4096)); };
  KCTRY(launch_timed(c, KT_GAP_SORT, kc_gap_sort_kernel, waves_grid(n_alns), dim3(GAP_TPB), 0, a));
  HIPCHK(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t nlist = h[GPS_NLIST];
  if (nlist) {
    // rows a lane holds: a 150-base read takes three, 1024 bases sixteen
    const uint64_t rows = (h_als[ALS_MAX_LEN] + 63) / 64;
    auto go = [&](auto r) {
      return launch_timed(c, KT_GAP_DP, kc_gap_dp_kernel<decltype(r)::value>, waves_grid(nlist), dim3(GAP_TPB), 0, a, nlist);
    };
    if (rows <= 1)
      KCTRY(go(int_c<1>{}));
    else if (rows <= 3)
      KCTRY(go(int_c<3>{}));
    else if (rows <= 8)
      KCTRY(go(int_c<8>{}));
    else
      KCTRY(go(int_c<16>{}));
    HIPCHK(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  }
  if (!on_device) HIPCHK(hipMemcpyAsync(out, d_out, n_alns * sizeof(kc_gap_aln), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (stats) {
    stats->records = n_alns;
    stats->exact = h[GPS_EXACT];
    stats->dp = h[GPS_DP];
    stats->none = h[GPS_NONE];
    stats->cells = h[GPS_CELLS];
    stats->score_sum = h[GPS_SCORE_SUM];
  }
  return KC_OK;
}

extern "C" int kc_align_gapped(kc_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, const kc_read_aln *alns,
                               uint64_t n_alns, int on_device, uint32_t pad, const kc_aln_scores *scores, uint32_t flags, kc_gap_aln *out,
                               kc_gap_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!scores || !out) return KC_ERR_INVALID_ARG;
  if (scores->match < 1 || scores->match > 9 || scores->mismatch > 9 || scores->ambiguity > 9 || scores->gap_ext < 1 ||
      scores->gap_ext > scores->gap_open || scores->gap_open > 9) {
    snprintf(g_last_error, sizeof(g_last_error),
             "kc_align_gapped: scores %u %u %u %u %u outside 1 <= match <= 9, mismatch, ambiguity <= 9, 1 <= gap_ext <= gap_open <= 9",
             scores->match, scores->mismatch, scores->gap_open, scores->gap_ext, scores->ambiguity);
    return KC_ERR_INVALID_ARG;
  }
  if (pad > KC_GAP_MAX_PAD || (flags & ~KC_GAP_ALWAYS_DP)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_align_gapped: pad %u over %d or unknown flags 0x%x", pad, KC_GAP_MAX_PAD, flags);
    return KC_ERR_INVALID_ARG;
  }
  if (!c) return KC_ERR_INVALID_ARG;
  if ((nreads && !offsets) || (n_alns && !alns) || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)out) & 15)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_align_gapped: a device record array is 16-byte aligned");
    return KC_ERR_INVALID_ARG;
  }
  if (!c->ai_ready) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_align_gapped: no contig index (kc_ctg_index_build)");
    return KC_ERR_STATE;
  }
  if (n_alns > 0xFFFFFFFFull) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_align_gapped: %llu records, the list holds 32-bit indices", (unsigned long long)n_alns);
    return KC_ERR_CAPACITY;
  }
  if (!n_alns) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return KC_OK;
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  AlignBufs b;
  const int rc = gap_run(c, b, bases, offsets, nreads, alns, n_alns, on_device, pad, scores, flags, out, stats);
  if (rc) (void)hipStreamSynchronize(c->stream);
  b.release();
  return rc;
}
