// kc_api_align.hpp -- kc_ctg_index_build, kc_ctg_index_clear, kc_align_reads (kernels in kc_align.hpp).  Part of
// kc_api.hip's translation unit, like kc_api_unitig.hpp.

static_assert(sizeof(kc_read_aln) == 32, "a record is two 16-byte stores");
static_assert(KC_ALIGN_MAX_READ_LEN == ALIGN_MAX_READ_LEN, "the header's limit is the kernels'");

template <int NL>
static int ctg_index_run(kc_ctx *c, CallBufs &b, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, int on_device,
                         AlignIndex &ix, kc_ctg_index_stats *stats) {
  // the table: at most half full whatever the block holds (a block of n bytes has fewer than n windows)
  const uint64_t cap = next_pow2(std::max<uint64_t>(2 * nbytes, 64));
  uint8_t *d_seqs;
  uint32_t *d_offs;
  uint64_t *d_slots, *d_in_offs, *d_status;
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    d_slots = m.take<uint64_t>(cap);
    d_offs = m.take<uint32_t>(n_ctgs + 1);
    d_seqs = m.take<uint8_t>(nbytes + 1);
    return m.used;
  };
  auto scratch = [&](uint8_t *base) {
    Carver m{base, 0};
    d_status = m.take<uint64_t>(AIS_COUNT);
    d_in_offs = m.take<uint64_t>(n_ctgs + 1);
    return m.used;
  };
  KCTRY(b.carve(layout));
  KCTRY(b.carve(scratch));
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (nbytes) HIPCHK(hipMemcpyAsync(d_seqs, seqs, nbytes, kind, c->stream));
  HIPCHK(hipMemcpyAsync(d_in_offs, offsets, (n_ctgs + 1) * 8, kind, c->stream));
  HIPCHK(hipMemsetAsync(d_status, 0, AIS_COUNT * 8, c->stream));
  HIPCHK(hipMemsetAsync(d_slots, 0, cap * 8, c->stream));
  const dim3 tpb(256);
  KCTRY(launch_timed(c, KT_ALIGN_CHECK, kc_align_check_kernel, blocks_for(std::max(nbytes, n_ctgs + 1)), tpb, 0, (const uint8_t *)d_seqs, nbytes,
                     (const uint64_t *)d_in_offs, n_ctgs, d_offs, d_status));
  uint64_t h[AIS_COUNT];
  KCTRY(read_back(c, h, d_status));
  if (h[AIS_BAD_BASE]) return fail(KC_ERR_BAD_BASE, "kc_ctg_index_build: a byte outside ACGTN and '_' in the block");
  if (h[AIS_BAD_OFFSETS] || h[AIS_SEPARATORS] != n_ctgs)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_index_build: the offsets of %llu contigs do not match the block's %llu separators",
                (unsigned long long)n_ctgs, (unsigned long long)h[AIS_SEPARATORS]);
  if (nbytes) {
    KCTRY(launch_timed(c, KT_ALIGN_INDEX, kc_align_index_kernel<NL>, blocks_for(nbytes), tpb, 0, (const uint8_t *)d_seqs, (uint32_t)nbytes, c->k,
                       d_slots, cap - 1, d_status));
    KCTRY(launch_timed(c, KT_ALIGN_SWEEP, kc_align_sweep_kernel, blocks_for(cap), tpb, 0, (const uint64_t *)d_slots, cap, d_status));
    KCTRY(read_back(c, h, d_status));
  }
  ix.seqs = d_seqs;
  ix.offs = d_offs;
  ix.slots = d_slots;
  ix.mask = cap - 1;
  ix.n_ctgs = (uint32_t)n_ctgs;
  if (stats) {
    stats->contigs = n_ctgs;
    stats->bases = nbytes - n_ctgs;
    stats->windows = h[AIS_WINDOWS];
    stats->seeds = h[AIS_SEEDS];
    stats->repeated = h[AIS_REPEATED];
  }
  return KC_OK;
}

extern "C" int kc_ctg_index_clear(kc_ctx *c) {
  if (!c) return KC_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipStreamSynchronize(c->stream));
  free_align_index(c);
  return KC_OK;
}

extern "C" int kc_ctg_index_build(kc_ctx *c, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, int on_device,
                                  kc_ctg_index_stats *stats) {
  if (!c || !offsets || (nbytes && !seqs)) return KC_ERR_INVALID_ARG;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (nbytes >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_ctg_index_build: a block of %llu bytes, slots hold 32-bit positions (fewer than 2^31 bytes)",
                (unsigned long long)nbytes);
  if (n_ctgs > nbytes) {  // every contig has its separator
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_index_build: %llu contigs in %llu bytes", (unsigned long long)n_ctgs, (unsigned long long)nbytes);
  }
  return call_with_bufs(c, [&](CallBufs &b) {
    AlignIndex ix;
    memset(&ix, 0, sizeof(ix));
    KCTRY(with_nl(c, [&](auto nl) { return ctg_index_run<nl>(c, b, seqs, nbytes, offsets, n_ctgs, on_device, ix, stats); }));
    // only now: had it failed, the earlier index, if any, would answer as before
    free_align_index(c);
    b.hand_over(ix.slots, c->d_ai);  // the table is the front of the index's allocation, which the context keeps
    c->ai = ix;
    c->ai_nbytes = nbytes;
    c->ai_ready = true;
    return (int)KC_OK;
  });
}

template <int NL>
static int align_launch(kc_ctx *c, int kind, uint32_t wpl, dim3 grid, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads,
                        uint32_t seed_space, uint32_t max_mismatches, uint64_t *first, uint4 *alns, uint64_t *st) {
  auto go = [&](auto w) {
    return launch_timed(c, kind, kc_align_reads_kernel<NL, decltype(w)::value>, grid, dim3(ALIGN_TPB), 0, c->ai, bases, offsets, nreads, c->k,
                        seed_space, max_mismatches, first, alns, st);
  };
  // windows a lane holds: a 150-base read has at most 148, three a lane; 1024 bases at most 1022, sixteen
  if (wpl <= 1) return go(int_c<1>{});
  if (wpl <= 3) return go(int_c<3>{});
  if (wpl <= 8) return go(int_c<8>{});
  return go(int_c<16>{});
}

static int align_run(kc_ctx *c, CallBufs &b, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, int on_device, uint32_t seed_space,
                     uint32_t max_mismatches, kc_read_aln *alns, uint64_t capacity, uint64_t *read_first, uint64_t *n_alns,
                     kc_align_stats *stats) {
  uint64_t *d_st, *d_first;
  StagedIn<uint64_t> offs = staged_offsets(offsets, nreads, on_device);
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    d_st = m.take<uint64_t>(ALS_COUNT);
    d_first = m.take<uint64_t>(nreads + 1);  // the reads' counts, scanned in place; the total behind them
    offs.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  const uint64_t *d_offs = offs.d;
  HIPCHK(hipMemsetAsync(d_st, 0, ALS_COUNT * 8, c->stream));
  uint64_t max_len, last;
  KCTRY(check_read_lengths(c, KT_ALIGN_LENGTHS, "kc_align_reads", d_offs, nreads, d_st, &max_len, &last));
  if (last && !bases) return KC_ERR_INVALID_ARG;
  const uint8_t *d_bases = bases;
  if (!on_device && last) KCTRY(upload_reads(c, b, bases, last, &d_bases));
  const uint64_t k = (uint64_t)c->k;
  const uint64_t starts = max_len >= k ? (max_len - k) / seed_space + 1 : 0;
  const uint32_t wpl = (uint32_t)((starts + 63) / 64);
  const dim3 grid((unsigned)((nreads + ALIGN_WAVES - 1) / ALIGN_WAVES));
  auto pass = [&](int kind, uint4 *out) {
    return with_nl(c, [&](auto nl) {
      return align_launch<nl>(c, kind, wpl, grid, d_bases, d_offs, nreads, seed_space, max_mismatches, d_first, out, d_st);
    });
  };
  KCTRY(pass(KT_ALIGN_COUNT, nullptr));
  KCTRY(launch_timed(c, KT_ALIGN_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{d_first}}, nreads, d_st + ALS_TOTAL));
  HIPCHK(hipMemcpyAsync(d_first + nreads, d_st + ALS_TOTAL, 8, hipMemcpyDeviceToDevice, c->stream));
  uint64_t h[ALS_COUNT];
  KCTRY(read_back(c, h, d_st));
  const uint64_t total = h[ALS_TOTAL];
  *n_alns = total;
  if (stats) {
    stats->reads = nreads;
    stats->reads_aligned = h[ALS_READS_ALIGNED];
    stats->windows = h[ALS_WINDOWS];
    stats->seed_hits = h[ALS_SEED_HITS];
    stats->repeated_hits = h[ALS_REPEATED_HITS];
    stats->alignments = total;
    stats->perfect = h[ALS_PERFECT];
  }
  if (!alns) return KC_OK;  // a size query
  if (total > capacity)
    return fail(KC_ERR_CAPACITY, "kc_align_reads: %llu alignments, the array holds %llu", (unsigned long long)total, (unsigned long long)capacity);
  uint4 *d_alns = (uint4 *)alns;
  if (!on_device) KCTRY(b.alloc(&d_alns, total * sizeof(kc_read_aln)));
  if (total) KCTRY(pass(KT_ALIGN_WRITE, d_alns));
  if (!on_device && total) HIPCHK(hipMemcpyAsync(alns, d_alns, total * sizeof(kc_read_aln), hipMemcpyDeviceToHost, c->stream));
  if (read_first)
    HIPCHK(hipMemcpyAsync(read_first, d_first, (nreads + 1) * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

extern "C" int kc_align_reads(kc_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, int on_device, uint32_t seed_space,
                              uint32_t max_mismatches, kc_read_aln *alns, uint64_t capacity, uint64_t *read_first, uint64_t *n_alns,
                              kc_align_stats *stats) {
  if (!c || !n_alns || !seed_space || (nreads && !offsets) || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && ((uintptr_t)alns & 15)) return misaligned_records("kc_align_reads");
  *n_alns = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!c->ai_ready) return no_ctg_index("kc_align_reads");
  if (!nreads) {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (alns && read_first) {  // the one entry of no reads: the total
      if (on_device) {
        HIPCHK(hipMemsetAsync(read_first, 0, 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
      } else {
        read_first[0] = 0;
      }
    }
    return KC_OK;
  }
  return call_with_bufs(c, [&](CallBufs &b) {
    return align_run(c, b, bases, offsets, nreads, on_device, seed_space, max_mismatches, alns, capacity, read_first, n_alns, stats);
  });
}
