// kc_api_break.hpp -- kc_ctg_break (kernels in kc_break.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_polish.hpp; the checks and the verdicts are kc_api_call.hpp's, the protocol kc_api_dedup.hpp's.
//
// The entry point is declared in include/kcount_mi355_break.h, inside that header's extern "C" block, and defined here
// without a linkage specifier of its own, as kc_api_polish.hpp does: tests/test_poisoned_scratch_coverage.py finds entry points
// by the specifier's text and holds a closed list.  tests/test_entry_point_coverage_break.py reads the fourth header instead.

static_assert(sizeof(kc_break_params) == 32 && sizeof(kc_break_piece) == 16 && sizeof(kc_break_rec) == 32 && sizeof(kc_break_stats) == 128,
              "the header's layouts");
static_assert(KC_BREAK_ONE_MATE == BREAK_ONE_MATE, "the header's constants are the kernels'");

struct BreakIo {
  const uint64_t *offsets;
  uint64_t nreads;
  const kc_gap_aln *alns;
  uint64_t n_alns;
  const kc_pair_rec *pairs;
  const uint16_t *depths;
  int on_device;
  uint8_t *seqs_out;
  uint64_t capacity;
  uint64_t *offsets_out;
  uint16_t *depths_out;
  kc_break_piece *pieces;
  kc_break_rec *breaks;
  uint64_t break_capacity;
  uint16_t *span_out, *disc_out;
  uint64_t *n_out, *nbytes_out;
  kc_break_stats *stats;
};

static int break_run(kc_ctx *c, CallBufs &b, const BreakIo &io, const kc_break_params &p) {
  const uint64_t nbytes = c->ai_nbytes, n_ctgs = c->ai.n_ctgs, nreads = io.nreads, n_alns = io.n_alns, npairs = nreads / 2;
  const uint64_t tiles = (nbytes + BREAK_TILE - 1) / BREAK_TILE;
  const bool dev = io.on_device != 0;
  BreakArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  LassmArgs la;
  memset(&la, 0, sizeof(la));
  uint64_t *d_als;
  StagedIn<uint64_t> offs = staged_offsets(io.offsets, nreads, dev);
  StagedIn<uint4> alns{io.alns, dev, n_alns * sizeof(kc_gap_aln)}, pairs{io.pairs, dev, npairs * sizeof(kc_pair_rec)};
  size_t zeroed = 0;  // the front of the scratch is counters and differences: one memset
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(BKS_COUNT);
    d.st = m.take<uint64_t>(DPS_COUNT);
    la.st = m.take<uint64_t>(LS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    a.span = m.take<uint32_t>(tiles * BREAK_TILE);
    a.disc = m.take<uint32_t>(tiles * BREAK_TILE);
    zeroed = m.used;
    a.wk = m.take<uint8_t>(tiles * BREAK_TILE);
    a.tsum_span = m.take<uint64_t>(tiles);
    a.tsum_disc = m.take<uint64_t>(tiles);
    a.tile_brk = m.take<uint64_t>(tiles);
    a.tile_lnw = m.take<uint32_t>(tiles);
    a.tile_lbase = m.take<uint32_t>(tiles);
    offs.reserve(m);
    alns.reserve(m);
    pairs.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(alns.upload(c));
  KCTRY(pairs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(la.st + LS_BAD_PAIR, 0xFF, 8, c->stream));
  // ---- the checks, a read, then a record, then a pair: nothing is stored through the caller's pointers before the last
  KCTRY(check_read_lengths(c, KT_BREAK_LENGTHS, "kc_ctg_break", offs.d, nreads, d_als));
  KCTRY(check_read_records(c, d, KT_BREAK_CHECK, "kc_ctg_break", alns.d, n_alns, offs.d, nreads));
  la.pairs = pairs.d;
  la.alns = alns.d;
  la.n_alns = n_alns;
  la.nreads = nreads;
  KCTRY(check_pairs(c, la, npairs, KT_BREAK_PAIR_CHECK, "kc_ctg_break"));
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.nbytes = (uint32_t)nbytes;
  a.alns = alns.d;
  a.pairs = pairs.d;
  a.offsets = offs.d;
  a.npairs = npairs;
  a.max_insert = p.max_insert;
  a.max_span = p.max_span;
  a.min_disc = p.min_disc;
  a.margin = p.margin;
  a.min_run = p.min_run;
  a.flags = p.flags;
  const dim3 grid((unsigned)tiles), tpb(BREAK_TPB);
  if (npairs) KCTRY(launch_timed(c, KT_BREAK_MARK, kc_break_mark_kernel, blocks_for(npairs, BREAK_TPB), tpb, 0, a));
  if (tiles) {
    KCTRY(launch_timed(c, KT_BREAK_TILE_SUMS, kc_break_tile_sums_kernel, grid, tpb, 0, a));
    KCTRY(launch_timed(c, KT_BREAK_SCAN, kc_scan_kernel<2>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<2>{{a.tsum_span, a.tsum_disc}}, tiles,
                       a.st + BKS_SCAN_SPAN));
    KCTRY(launch_timed(c, KT_BREAK_RESCAN, kc_break_rescan_kernel, grid, tpb, 0, a));
    KCTRY(launch_timed(c, KT_BREAK_TILE_MAX, kc_break_tile_max_kernel, dim3(1), dim3(BREAK_MAX_TPB), 0, (const uint32_t *)a.tile_lnw, a.tile_lbase,
                       tiles));
    // the count pass: one break too many is an error before anything is stored
    KCTRY(launch_timed(c, KT_BREAK_RUNS_COUNT, kc_break_runs_kernel<false>, grid, tpb, 0, a));
    KCTRY(launch_timed(c, KT_BREAK_RUNS_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.tile_brk}}, tiles,
                       a.st + BKS_SCAN_BREAKS));
  }
  uint64_t h[BKS_COUNT];
  KCTRY(read_back(c, h, a.st));
  const uint64_t nb = h[BKS_SCAN_BREAKS];
  if (nb != h[BKS_BREAKS] || nb > nbytes)
    return fail(KC_ERR_STATE, "kc_ctg_break: the scan gives %llu breaks, the sum %llu", (unsigned long long)nb, (unsigned long long)h[BKS_BREAKS]);
  if (io.breaks && nb > io.break_capacity)
    return fail(KC_ERR_CAPACITY, "kc_ctg_break: %llu breaks, room for %llu", (unsigned long long)nb, (unsigned long long)io.break_capacity);
  const uint64_t n_out = n_ctgs + nb, total = nbytes + nb;
  const bool fits = io.seqs_out && io.capacity >= total;
  // ---- out: from here on the caller's arrays are written, if the block fits
  StagedOut<uint8_t> seqs{io.seqs_out, dev, (size_t)total};
  StagedOut<uint64_t> offsets{io.offsets_out, dev, (size_t)(n_out + 1) * 8};
  StagedOut<uint16_t> depths{io.depths ? io.depths_out : nullptr, dev, (size_t)total * 2};
  StagedOut<uint4> pieces{io.pieces, dev, (size_t)n_out * sizeof(kc_break_piece)}, recs{io.breaks, dev, (size_t)nb * sizeof(kc_break_rec)};
  StagedOut<uint16_t> span{io.span_out, dev, (size_t)nbytes * 2}, disc{io.disc_out, dev, (size_t)nbytes * 2};
  StagedIn<uint16_t> din{io.depths, dev, (size_t)nbytes * 2, nbytes != 0};
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.binfo = m.take<uint4>(nb);
    seqs.reserve(m, fits);
    offsets.reserve(m, fits);
    depths.reserve(m, fits);
    pieces.reserve(m, fits);
    recs.reserve(m, fits);
    span.reserve(m, fits);
    disc.reserve(m, fits);
    din.reserve(m, fits && depths.dst != nullptr);
    return m.used;
  }));
  a.n_breaks = (uint32_t)nb;
  a.pieces = pieces.d;
  a.breaks = recs.d;
  a.offsets_out = offsets.d;
  if (nb) KCTRY(launch_timed(c, KT_BREAK_RUNS_WRITE, kc_break_runs_kernel<true>, grid, tpb, 0, a));
  if (n_ctgs)
    KCTRY(launch_timed(c, KT_BREAK_RECORDS, kc_break_records_kernel, blocks_for(n_out + 1, BREAK_TPB), tpb, 0, a));
  else if (offsets.d)
    HIPCHK(hipMemsetAsync(offsets.d, 0, 8, c->stream));
  if (fits && total) {
    BreakCopy g{c->ai.seqs, seqs.d, a.binfo, (uint32_t)nb, total, nbytes};
    KCTRY(launch_timed(c, KT_BREAK_GATHER, kc_break_gather_kernel<1>, blocks_for((total + 15 + 15) / 16, BREAK_TPB), tpb, 0, g));
    if (depths.d) {
      KCTRY(din.upload(c));
      g.src = (const uint8_t *)din.d;
      g.dst = (uint8_t *)depths.d;
      KCTRY(launch_timed(c, KT_BREAK_GATHER_DEPTHS, kc_break_gather_kernel<2>, blocks_for((2 * total + 15 + 15) / 16, BREAK_TPB), tpb, 0, g));
    }
    const dim3 per8 = blocks_for((nbytes + BREAK_ITEMS - 1) / BREAK_ITEMS, BREAK_TPB);
    if (span.d) KCTRY(launch_timed(c, KT_BREAK_TRACKS, kc_break_tracks_kernel, per8, tpb, 0, (const uint32_t *)a.span, span.d, (uint32_t)nbytes));
    if (disc.d) KCTRY(launch_timed(c, KT_BREAK_TRACKS, kc_break_tracks_kernel, per8, tpb, 0, (const uint32_t *)a.disc, disc.d, (uint32_t)nbytes));
  }
  KCTRY(seqs.download(c));
  KCTRY(offsets.download(c));
  KCTRY(depths.download(c));
  KCTRY(pieces.download(c));
  KCTRY(recs.download(c));
  KCTRY(span.download(c));
  KCTRY(disc.download(c));
  uint64_t broken = 0;
  KCTRY(read_back(c, &broken, a.st + BKS_BROKEN, 1));
  *io.n_out = n_out;
  *io.nbytes_out = total;
  if (io.stats) {
    kc_break_stats s;
    memset(&s, 0, sizeof(s));
    s.spanning = h[BKS_SPANNING];
    s.discordant_pairs = h[BKS_DISC_PAIRS];
    s.one_mate = h[BKS_ONE];
    s.none = h[BKS_NONE];
    s.pairs = npairs;
    s.disc_mates = h[BKS_DISC_MATES];
    s.empty_intervals = h[BKS_EMPTY];
    s.span_sum = h[BKS_SPAN_SUM];
    s.disc_sum = h[BKS_DISC_SUM];
    s.columns = (uint32_t)(nbytes - n_ctgs);
    s.interior = (uint32_t)h[BKS_INTERIOR];
    s.weak = (uint32_t)h[BKS_WEAK];
    s.runs = (uint32_t)h[BKS_RUNS];
    s.short_runs = (uint32_t)h[BKS_SHORT];
    s.breaks = (uint32_t)nb;
    s.broken_contigs = (uint32_t)broken;
    s.pieces = (uint32_t)n_out;
    *io.stats = s;
  }
  if (io.seqs_out && !fits)
    return fail(KC_ERR_CAPACITY, "kc_ctg_break: %llu bytes, the array holds %llu", (unsigned long long)total, (unsigned long long)io.capacity);
  return KC_OK;
}

int kc_ctg_break(kc_ctx *c, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs,
                 const uint16_t *depths, int on_device, const kc_break_params *p, uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out,
                 uint16_t *depths_out, kc_break_piece *pieces, kc_break_rec *breaks, uint64_t break_capacity, uint16_t *span_out, uint16_t *disc_out,
                 uint64_t *n_out, uint64_t *nbytes_out, kc_break_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_out || !nbytes_out) return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: %s is NULL", !p ? "params" : !n_out ? "n_out" : "nbytes_out");
  if (p->flags & ~KC_BREAK_ONE_MATE) return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: unknown flags 0x%x", p->flags & ~KC_BREAK_ONE_MATE);
  for (int i = 0; i < 2; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (p->max_insert < 1 || p->max_insert > KC_INSERT_MAX)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: max_insert %u outside 1 .. %d", p->max_insert, KC_INSERT_MAX);
  if (!p->margin) return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: margin is 0, at least 1");
  if (!p->min_run) return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: min_run is 0, at least 1");
  if (nreads & 1)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: %llu reads are no pairs (reads 2p and 2p + 1 are mates)", (unsigned long long)nreads);
  if (!c) return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: ctx is NULL");
  if ((nreads && !offsets) || (n_alns && !alns) || (nreads && !pairs))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: %s is NULL", (nreads && !offsets) ? "offsets" : (n_alns && !alns) ? "alns" : "pairs");
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs | (uintptr_t)pieces | (uintptr_t)breaks) & 15)) return misaligned_records("kc_ctg_break");
  if (on_device && ((((uintptr_t)offsets | (uintptr_t)offsets_out) & 7) ||
                    (((uintptr_t)depths | (uintptr_t)depths_out | (uintptr_t)span_out | (uintptr_t)disc_out) & 1)))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_break: device offsets are 8-byte aligned, depths and tracks 2-byte");
  if (!c->ai_ready) return no_ctg_index("kc_ctg_break");
  if (nreads > 0xFFFFFFFFull || n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_ctg_break: %llu reads and %llu records, an index of either takes 32 bits", (unsigned long long)nreads,
                (unsigned long long)n_alns);
  const BreakIo io{offsets, nreads, alns, n_alns, pairs, depths, on_device, seqs_out, capacity, offsets_out, depths_out, pieces, breaks,
                   break_capacity, span_out, disc_out, n_out, nbytes_out, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return break_run(c, b, io, *p); });
}
