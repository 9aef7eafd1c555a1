// kc_api_kdepth.hpp -- kc_seq_kmer_depths and kc_count_spectrum (kernels in kc_kdepth.hpp).  Part of kc_api.hip's
// translation unit, behind kc_api_dedup.hpp; the index is kc_lookup's (ensure_index).
//
// The two entry points are defined without a linkage specifier of their own: include/kcount_mi355.h declares them inside its
// extern "C" block, and a definition takes the linkage of the declaration before it.  tests/test_poisoned_scratch_coverage.py
// finds entry points by the specifier's text and holds a closed list of them; tests/test_entry_point_coverage_all.py reads
// the header instead, so these two, and whatever comes later, are held to the same rule whatever their spelling.

static_assert(sizeof(kc_kdepth_params) == 32 && sizeof(kc_kdepth_rec) == 32 && sizeof(kc_kdepth_stats) == 64 && sizeof(kc_spectrum_stats) == 64,
              "the header's layouts");
static_assert(offsetof(kc_kdepth_rec, windows) == 8 && offsetof(kc_kdepth_rec, solid) == 16 && offsetof(kc_kdepth_rec, min_count) == 20 &&
                  offsetof(kc_kdepth_rec, mean) == 24,
              "kc_ktrack_records_kernel writes these");
static_assert(KC_SPECTRUM_BINS == SPECT_BINS && SPS_COUNT * 8 == sizeof(kc_spectrum_stats), "the header's constants are the kernels'");

struct KdepthIo {
  const uint8_t *seqs;
  uint64_t nbytes;
  const uint64_t *offsets;
  uint64_t nseqs;
  int on_device;
  uint16_t *track;
  kc_kdepth_rec *recs;
  kc_kdepth_stats *stats;
};

template <int NL>
static int kdepth_run(kc_ctx *c, CallBufs &b, const KdepthIo &io, const kc_kdepth_params &p) {
  const uint64_t n = io.nseqs, nbytes = io.nbytes;
  const bool dev = io.on_device != 0, fill = (p.flags & KC_KDEPTH_FILL_MEAN) != 0;
  const bool per_seq = io.recs || (fill && io.track);
  KCTRY(ensure_index<NL>(c));
  KtrackArgs a;
  memset(&a, 0, sizeof(a));
  StagedIn<uint8_t> blk{io.seqs, dev, (size_t)nbytes};
  StagedIn<uint64_t> offs{io.offsets, dev, (size_t)(n + 1) * 8};
  StagedOut<uint16_t> track{io.track, dev, (size_t)nbytes * 2};
  StagedOut<uint4> recs{io.recs, dev, (size_t)n * sizeof(kc_kdepth_rec)};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(KTS_COUNT);
    if (per_seq) a.acc = m.take<KtrackAcc>(n);
    zeroed = m.used;
    if (fill && io.track) a.mean = m.take<uint16_t>(n);
    blk.reserve(m);
    offs.reserve(m);
    track.reserve(m);
    recs.reserve(m);
    return m.used;
  }));
  KCTRY(blk.upload(c));
  KCTRY(offs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(a.st, 0xFF, 2 * 8, c->stream));  // KTS_BAD, KTS_LONG: the lowest index, all ones for none
  // ---- the check: nothing is stored through the caller's pointers before its verdict
  KCTRY(launch_timed(c, KT_KTRACK_OFFSETS, kc_ktrack_offsets_kernel, blocks_for(n, KT_TPB), dim3(KT_TPB), 0, (const uint64_t *)offs.d, n, nbytes, a.st));
  uint64_t h[KTS_COUNT];
  KCTRY(read_back(c, h, a.st));
  if (h[KTS_BAD] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: the offsets decrease behind sequence %llu", (unsigned long long)h[KTS_BAD]);
  if (h[KTS_ENDS])
    return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: the offsets of %llu sequences do not %s", (unsigned long long)n,
                (h[KTS_ENDS] & 1) ? "start at 0" : "end at nbytes");
  if (h[KTS_LONG] != ~0ull)
    return fail(KC_ERR_CAPACITY, "kc_seq_kmer_depths: sequence %llu has 2^32 bytes or more", (unsigned long long)h[KTS_LONG]);
  a.seqs = blk.d;
  a.nbytes = nbytes;
  a.offs = offs.d;
  a.n = (uint32_t)n;
  a.k = c->k;
  a.solid = std::max(p.min_count, 1u);
  a.index = c->d_index;
  a.mask = c->index_cap - 1;
  a.keys = c->d_out_keys;
  a.counts = c->d_out_counts;
  a.track = track.d;
  a.recs = recs.d;
  const dim3 tpb(KT_TPB), lanes = blocks_for((nbytes + KT_RUN - 1) / KT_RUN, KT_TPB);
  if (fill)
    KCTRY(launch_timed(c, KT_KTRACK_WINDOWS_FILL, kc_ktrack_windows_kernel<NL, true>, lanes, tpb, 0, a));
  else
    KCTRY(launch_timed(c, KT_KTRACK_WINDOWS, kc_ktrack_windows_kernel<NL, false>, lanes, tpb, 0, a));
  if (per_seq) KCTRY(launch_timed(c, KT_KTRACK_RECORDS, kc_ktrack_records_kernel, blocks_for(n, KT_TPB), tpb, 0, a));
  if (fill && a.track)
    KCTRY(launch_timed(c, KT_KTRACK_FILL, kc_ktrack_fill_kernel, blocks_for((nbytes + KT_FILL_ITEMS - 1) / KT_FILL_ITEMS, KT_TPB), tpb, 0, a));
  KCTRY(track.download(c));
  KCTRY(recs.download(c));
  KCTRY(read_back(c, h, a.st));
  if (io.stats) {
    kc_kdepth_stats s;
    memset(&s, 0, sizeof(s));
    s.seqs = n;
    s.bytes = nbytes;
    s.windows = h[KTS_WINDOWS];
    s.present = h[KTS_PRESENT];
    s.solid = h[KTS_SOLID];
    s.sum = h[KTS_SUM];
    s.longest = h[KTS_LONGEST];
    *io.stats = s;
  }
  return KC_OK;
}

// no sequences or no bytes: zero stats, zero records, and no device work beyond clearing a device caller's arrays
static int kdepth_nothing(kc_ctx *c, const KdepthIo &io) {
  if (io.on_device) {
    if (io.track && io.nbytes) HIPCHK(hipMemsetAsync(io.track, 0, io.nbytes * 2, c->stream));
    if (io.recs && io.nseqs) HIPCHK(hipMemsetAsync(io.recs, 0, io.nseqs * sizeof(kc_kdepth_rec), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    if (io.track && io.nbytes) memset(io.track, 0, io.nbytes * 2);
    if (io.recs && io.nseqs) memset(io.recs, 0, io.nseqs * sizeof(kc_kdepth_rec));
  }
  if (io.stats) memset(io.stats, 0, sizeof(*io.stats));
  return KC_OK;
}

int kc_seq_kmer_depths(kc_ctx *c, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t nseqs, int on_device,
                       const kc_kdepth_params *p, uint16_t *track, kc_kdepth_rec *recs, kc_kdepth_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !offsets) return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: %s is NULL", !p ? "params" : "offsets");
  if (!seqs && nbytes) return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: seqs is NULL with %llu bytes", (unsigned long long)nbytes);
  if (p->flags & ~KC_KDEPTH_FILL_MEAN) return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: unknown flags 0x%x", p->flags & ~KC_KDEPTH_FILL_MEAN);
  for (int i = 0; i < 6; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (p->min_count > 65535u) return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: min_count is %u, at most 65535", p->min_count);
  if (!c) return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: ctx is NULL");
  if (nseqs >= (1ull << 32)) return fail(KC_ERR_CAPACITY, "kc_seq_kmer_depths: %llu sequences, at most 2^32 - 1", (unsigned long long)nseqs);
  if (on_device && (((uintptr_t)recs) & 15)) return misaligned_records("kc_seq_kmer_depths");
  if (on_device && ((((uintptr_t)offsets) & 7) || (((uintptr_t)track) & 1)))
    return fail(KC_ERR_INVALID_ARG, "kc_seq_kmer_depths: device offsets are 8-byte aligned, the track 2-byte");
  if (!c->finalized) return fail(KC_ERR_STATE, "kc_seq_kmer_depths: no results (kc_finalize)");
  const KdepthIo io{seqs, nbytes, offsets, nseqs, on_device, track, recs, stats};
  return call_with_bufs(c, [&](CallBufs &b) {
    if (!nseqs || !nbytes) return kdepth_nothing(c, io);
    return with_nl(c, [&](auto nl) { return kdepth_run<nl>(c, b, io, *p); });
  });
}

int kc_count_spectrum(kc_ctx *c, uint64_t *hist, int on_device, kc_spectrum_stats *stats) {
  if (!hist && !stats) return fail(KC_ERR_INVALID_ARG, "kc_count_spectrum: hist and stats are both NULL");
  if (!c) return fail(KC_ERR_INVALID_ARG, "kc_count_spectrum: ctx is NULL");
  if (on_device && (((uintptr_t)hist) & 7)) return fail(KC_ERR_INVALID_ARG, "kc_count_spectrum: a device hist is 8-byte aligned");
  if (!c->finalized) return fail(KC_ERR_STATE, "kc_count_spectrum: no results (kc_finalize)");
  return call_with_bufs(c, [&](CallBufs &b) {
    uint64_t *d_st, *d_hist = on_device ? hist : nullptr;
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      d_st = m.take<uint64_t>(SPS_COUNT);
      if (!on_device || !hist) d_hist = m.take<uint64_t>(SPECT_BINS);
      return m.used;
    }));
    HIPCHK(hipMemsetAsync(d_hist, 0, SPECT_BINS * 8, c->stream));
    if (c->out_n) {
      // a few workgroups a compute unit: each flushes its own LDS bins once
      const uint64_t want = (c->out_n + SPECT_TPB * SPECT_ITEMS - 1) / (SPECT_TPB * SPECT_ITEMS);
      const dim3 grid((unsigned)std::min<uint64_t>(want, (uint64_t)std::max(c->num_cus, 1) * 8));
      KCTRY(launch_timed(c, KT_SPECT_HIST, kc_spect_hist_kernel, grid, dim3(SPECT_TPB), 0, (const uint16_t *)c->d_out_counts, c->out_n, d_hist));
    }
    KCTRY(launch_timed(c, KT_SPECT_STATS, kc_spect_stats_kernel, dim3(1), dim3(1024), 0, (const uint64_t *)d_hist, d_st));
    if (hist && !on_device) HIPCHK(hipMemcpyAsync(hist, d_hist, SPECT_BINS * 8, hipMemcpyDeviceToHost, c->stream));
    uint64_t h[SPS_COUNT];
    KCTRY(read_back(c, h, d_st));
    if (stats) {
      kc_spectrum_stats s;
      memset(&s, 0, sizeof(s));
      s.kmers = h[SPS_KMERS];
      s.sum_counts = h[SPS_SUM];
      s.max_count = h[SPS_MAX];
      s.mode_count = h[SPS_MODE];
      s.mode_kmers = h[SPS_MODE_KMERS];
      s.saturated = h[SPS_SATURATED];
      *stats = s;
    }
    return (int)KC_OK;
  });
}
