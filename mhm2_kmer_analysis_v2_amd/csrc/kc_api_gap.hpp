// kc_api_gap.hpp -- kc_align_gapped (kernels in kc_gap.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_align.hpp.

static_assert(sizeof(kc_gap_aln) == 32, "a record is two 16-byte stores");
static_assert(sizeof(kc_gap_stats) == 48, "six counters");
static_assert(KC_GAP_MAX_PAD == GAP_MAX_PAD && KC_GAP_ALWAYS_DP == GAP_ALWAYS_DP, "the header's constants are the kernels'");
static_assert(KC_GAP_EXACT == GAP_KIND_EXACT && KC_GAP_DP == GAP_KIND_DP && KC_GAP_NONE == GAP_KIND_NONE, "the header's kinds");

static int gap_run(kc_ctx *c, CallBufs &b, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, const kc_read_aln *alns,
                   uint64_t n_alns, int on_device, uint32_t pad, const kc_aln_scores *sc, uint32_t flags, kc_gap_aln *out,
                   kc_gap_stats *stats) {
  const bool dev = on_device != 0;
  uint64_t *d_st, *d_als, *d_list;
  StagedIn<uint64_t> offs = staged_offsets(offsets, nreads, dev);
  StagedIn<uint4> in{alns, dev, n_alns * sizeof(kc_read_aln)};
  StagedOut<uint4> recs{out, dev, n_alns * sizeof(kc_gap_aln)};
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    d_st = m.take<uint64_t>(GPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    d_list = m.take<uint64_t>(n_alns);
    offs.reserve(m);
    in.reserve(m);
    recs.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(in.upload(c));
  HIPCHK(hipMemsetAsync(d_st, 0, GPS_COUNT * 8, c->stream));
  HIPCHK(hipMemsetAsync(d_st + GPS_BAD, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d_als, 0, ALS_COUNT * 8, c->stream));
  uint64_t max_len, last;
  KCTRY(check_read_lengths(c, KT_GAP_LENGTHS, "kc_align_gapped", offs.d, nreads, d_als, &max_len, &last));
  if (last && !bases) return KC_ERR_INVALID_ARG;
  const uint8_t *d_bases = bases;
  if (!dev && last) KCTRY(upload_reads(c, b, bases, last, &d_bases));
  GapArgs a;
  a.ix = c->ai;
  a.bases = d_bases;
  a.offsets = offs.d;
  a.nreads = nreads;
  a.alns = in.d;
  a.n_alns = n_alns;
  a.out = recs.d;
  a.pad = pad;
  a.flags = flags;
  a.match = (int)sc->match;
  a.mismatch = (int)sc->mismatch;
  a.gap_open = (int)sc->gap_open;
  a.gap_ext = (int)sc->gap_ext;
  a.amb = (int)sc->ambiguity;
  a.list = d_list;
  a.st = d_st;
  KCTRY(launch_timed(c, KT_GAP_CHECK, kc_gap_check_kernel, blocks_for(n_alns), dim3(256), 0, a));
  uint64_t h[GPS_COUNT];
  KCTRY(read_back(c, h, d_st));
  if (h[GPS_BAD] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "kc_align_gapped: record %llu is not one kc_align_reads emits for these reads and this index",
                (unsigned long long)h[GPS_BAD]);
  // a wave per record, or a few records a wave once every compute unit is full
  auto waves_grid = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + GAP_WAVES - 1) / GAP_WAVES, 4096)); };
  KCTRY(launch_timed(c, KT_GAP_SORT, kc_gap_sort_kernel, waves_grid(n_alns), dim3(GAP_TPB), 0, a));
  KCTRY(read_back(c, h, d_st));
  const uint64_t nlist = h[GPS_NLIST];
  if (nlist) {
    // rows a lane holds: a 150-base read takes three, 1024 bases sixteen
    const uint64_t rows = (max_len + 63) / 64;
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
  KCTRY(recs.download(c));
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
      scores->gap_ext > scores->gap_open || scores->gap_open > 9)
    return fail(KC_ERR_INVALID_ARG,
                "kc_align_gapped: scores %u %u %u %u %u outside 1 <= match <= 9, mismatch, ambiguity <= 9, 1 <= gap_ext <= gap_open <= 9",
                scores->match, scores->mismatch, scores->gap_open, scores->gap_ext, scores->ambiguity);
  if (pad > KC_GAP_MAX_PAD || (flags & ~KC_GAP_ALWAYS_DP))
    return fail(KC_ERR_INVALID_ARG, "kc_align_gapped: pad %u over %d or unknown flags 0x%x", pad, KC_GAP_MAX_PAD, flags);
  if (!c) return KC_ERR_INVALID_ARG;
  if ((nreads && !offsets) || (n_alns && !alns) || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)out) & 15)) return misaligned_records("kc_align_gapped");
  if (!c->ai_ready) return no_ctg_index("kc_align_gapped");
  if (n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_align_gapped: %llu records, the list holds 32-bit indices", (unsigned long long)n_alns);
  if (!n_alns) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return KC_OK;
  }
  return call_with_bufs(c, [&](CallBufs &b) {
    return gap_run(c, b, bases, offsets, nreads, alns, n_alns, on_device, pad, scores, flags, out, stats);
  });
}
