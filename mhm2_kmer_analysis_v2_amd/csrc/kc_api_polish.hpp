// kc_api_polish.hpp -- kc_ctg_polish (kernels in kc_polish.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_correct.hpp; the checks are kc_api_call.hpp's, the radix passes kc_sort.hpp's as kc_api_shuffle.hpp uses them.
//
// The entry point is declared in include/kcount_mi355_polish.h, inside that header's extern "C" block, and defined here
// without a linkage specifier of its own, as kc_api_correct.hpp does: tests/test_poisoned_scratch_coverage.py finds entry points
// by the specifier's text and holds a closed list.  tests/test_entry_point_coverage_polish.py reads the third header instead.

static_assert(sizeof(kc_polish_params) == 32 && sizeof(kc_polish_ctg) == 32 && sizeof(kc_polish_fix) == 16 && sizeof(kc_polish_stats) == 128,
              "the header's layouts");
static_assert(sizeof(kc_polish_ctg) == PLC_WORDS * 4 && offsetof(kc_polish_ctg, placed) == PLC_PLACED * 4 &&
                  offsetof(kc_polish_ctg, changed) == PLC_CHANGED * 4 && offsetof(kc_polish_ctg, filled) == PLC_FILLED * 4 &&
                  offsetof(kc_polish_ctg, disputed) == PLC_DISPUTED * 4 && offsetof(kc_polish_ctg, thin) == PLC_THIN * 4 &&
                  offsetof(kc_polish_ctg, uncovered) == PLC_UNCOVERED * 4,
              "the kernels add into the record's own layout");
static_assert(offsetof(kc_polish_fix, ctg) == 4 && offsetof(kc_polish_fix, old_base) == 8 && offsetof(kc_polish_fix, new_base) == 9 &&
                  offsetof(kc_polish_fix, top) == 10 && offsetof(kc_polish_fix, tot) == 12 && offsetof(kc_polish_fix, pad) == 14,
              "polish_decide writes these");
static_assert(KC_POLISH_BEST_ONLY == POLISH_BEST_ONLY, "the header's constants are the kernels'");

struct PolishIo {
  const uint8_t *bases, *quals;
  const uint64_t *offsets;
  uint64_t nreads;
  const kc_gap_aln *alns;
  uint64_t n_alns;
  int on_device;
  uint8_t *out;
  uint16_t *counts;
  kc_polish_ctg *ctgs;
  kc_polish_fix *fixes;
  uint64_t fix_capacity;
  kc_polish_stats *stats;
};

static int polish_run(kc_ctx *c, CallBufs &b, const PolishIo &io, const kc_polish_params &p) {
  const uint64_t nbytes = c->ai_nbytes, n_ctgs = c->ai.n_ctgs, nreads = io.nreads, n_alns = io.n_alns;
  const uint64_t tiles = (nbytes + POLISH_TILE - 1) / POLISH_TILE, scan_tiles = (tiles + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  const uint64_t ntiles = (n_alns + SORT_TILE - 1) / SORT_TILE, ncnt = ntiles * SORT_DIGITS;
  const bool dev = io.on_device != 0, best_only = (p.flags & KC_POLISH_BEST_ONLY) != 0, gate = io.quals && p.min_qual;
  PolishArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  uint64_t *d_als, *kbuf[2] = {nullptr, nullptr}, *cnt = nullptr, *tile_base = nullptr;
  uint32_t *ibuf[2] = {nullptr, nullptr};
  StagedIn<uint64_t> offs = staged_offsets(io.offsets, nreads, dev);
  StagedIn<uint4> alns{io.alns, dev, n_alns * sizeof(kc_gap_aln)};
  StagedOut<uint8_t> out{io.out, dev, nbytes};
  StagedOut<uint16_t> counts{io.counts, dev, nbytes * 8};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(PLS_COUNT);
    d.st = m.take<uint64_t>(DPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    a.cacc = m.take<uint32_t>(n_ctgs * PLC_WORDS);
    d.best = m.take<uint64_t>(best_only ? nreads : 0);
    zeroed = m.used;
    kbuf[0] = m.take<uint64_t>(n_alns);
    kbuf[1] = m.take<uint64_t>(n_alns);
    ibuf[0] = m.take<uint32_t>(n_alns);
    ibuf[1] = m.take<uint32_t>(n_alns);
    cnt = m.take<uint64_t>(ncnt);
    a.lane_changed = m.take<uint8_t>(io.fixes ? tiles * POLISH_OUT_LANES : 0);
    a.tile_changed = m.take<uint64_t>(io.fixes ? tiles : 0);
    tile_base = m.take<uint64_t>(io.fixes ? scan_tiles : 0);
    offs.reserve(m);
    alns.reserve(m);
    out.reserve(m);
    counts.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(alns.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  // ---- the checks: nothing is stored through the caller's pointers before the last of them has passed
  uint64_t last = 0;
  KCTRY(check_read_lengths(c, KT_POLISH_LENGTHS, "kc_ctg_polish", offs.d, nreads, d_als, nullptr, &last));
  d.min_score = p.min_score;
  d.min_len = p.min_len;
  KCTRY(check_read_records(c, d, KT_POLISH_CHECK, "kc_ctg_polish", alns.d, n_alns, offs.d, nreads));
  if (last && !io.bases) return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: bases is NULL and the reads have %llu bytes", (unsigned long long)last);
  const uint8_t *d_bases = io.bases, *d_quals = gate ? io.quals : nullptr;
  if (!dev && last) {
    KCTRY(upload_reads(c, b, io.bases, last, &d_bases));
    if (gate) KCTRY(upload_reads(c, b, io.quals, last, &d_quals));
  }
  a.seqs = c->ai.seqs;
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.nbytes = (uint32_t)nbytes;
  a.bases = d_bases;
  a.quals = d_quals;
  a.offsets = offs.d;
  a.total = last;
  a.alns = alns.d;
  a.n_alns = n_alns;
  a.min_score = p.min_score;
  a.min_len = p.min_len;
  a.edge_clip = p.edge_clip;
  a.max_mismatches = p.max_mismatches;
  a.min_depth = p.min_depth;
  a.min_permille = p.min_permille;
  a.min_qual = p.min_qual;
  a.flags = p.flags;
  a.qual_offset = c->cfg.qual_offset;
  a.best = d.best;
  a.keys = kbuf[0];
  a.out = out.d;
  a.counts = counts.d;
  a.tile_base = tile_base;
  int passes = 0;
  if (n_alns) {
    if (best_only) KCTRY(launch_timed(c, KT_POLISH_BEST, kc_depth_best_kernel, blocks_for(n_alns), dim3(256), 0, d));
    KCTRY(launch_timed(c, KT_POLISH_PLACE, kc_polish_place_kernel, blocks_for(n_alns, POLISH_WAVES), dim3(POLISH_TPB), 0, a));
    // ---- one stable sort of the permutation over the significant bits of a block position; a record that is not
    // placed has all of them set, which no position has: 2^bits > nbytes
    const int bits = 64 - __builtin_clzll((unsigned long long)nbytes | 1ull);
    int cur = 0;
    const uint32_t *perm = nullptr;  // the identity until the first pass has run
    for (int shift = 0; shift < bits; shift += SORT_BITS) {
      const uint32_t mask = (1u << std::min(SORT_BITS, bits - shift)) - 1u;
      KCTRY(launch_timed(c, KT_POLISH_SORT_HIST, kc_sort_hist_kernel<false>, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)nullptr, 1, 0,
                         perm, kbuf[cur], n_alns, ntiles, shift, mask, cnt));
      KCTRY(launch_timed(c, KT_POLISH_SORT_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{cnt}}, ncnt, a.st + PLS_SORT_TOTAL));
      KCTRY(launch_timed(c, KT_POLISH_SORT_SCATTER, kc_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)kbuf[cur], perm,
                         kbuf[cur ^ 1], ibuf[cur ^ 1], n_alns, ntiles, shift, mask, (const uint64_t *)cnt));
      cur ^= 1;
      perm = ibuf[cur];
      passes++;
    }
    a.skeys = kbuf[cur];
    a.perm = perm;
  }
  // ---- the tiles: with fixes the count pass first, so that too many of them are found before anything is written
  const dim3 grid((unsigned)tiles), tpb(POLISH_TPB);
  uint64_t n_fixes = 0;
  uint4 *d_fixes = nullptr;
  if (io.fixes && tiles) {
    KCTRY(launch_timed(c, KT_POLISH_TILE_COUNT, kc_polish_tile_kernel<0>, grid, tpb, 0, a));
    KCTRY(tiled_scan(c, KT_POLISH_TILE_SCAN, KT_POLISH_SCAN, a.tile_changed, tiles, tile_base, a.st + PLS_FIXES));
    KCTRY(read_back(c, &n_fixes, a.st + PLS_FIXES, 1));
    if (n_fixes > io.fix_capacity)
      return fail(KC_ERR_CAPACITY, "kc_ctg_polish: %llu fixes, room for %llu", (unsigned long long)n_fixes, (unsigned long long)io.fix_capacity);
    d_fixes = (uint4 *)io.fixes;
    if (!dev) KCTRY(b.alloc(&d_fixes, n_fixes * sizeof(kc_polish_fix)));
  }
  // ---- out: from here on the caller's arrays are written
  a.fixes = n_fixes ? d_fixes : nullptr;
  if (tiles) KCTRY(launch_timed(c, KT_POLISH_TILE_WRITE, kc_polish_tile_kernel<1>, grid, tpb, 0, a));
  KCTRY(out.download(c));
  KCTRY(counts.download(c));
  if (io.ctgs && n_ctgs)
    HIPCHK(hipMemcpyAsync(io.ctgs, a.cacc, n_ctgs * sizeof(kc_polish_ctg), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  if (!dev && n_fixes) HIPCHK(hipMemcpyAsync(io.fixes, d_fixes, n_fixes * sizeof(kc_polish_fix), hipMemcpyDeviceToHost, c->stream));
  uint64_t h[PLS_COUNT];
  KCTRY(read_back(c, h, a.st));
  if (io.stats) {
    kc_polish_stats s;
    memset(&s, 0, sizeof(s));
    s.records = n_alns;
    s.none = h[PLS_NONE];
    s.filtered = h[PLS_FILTERED];
    s.not_best = h[PLS_NOT_BEST];
    s.unequal = h[PLS_UNEQUAL];
    s.divergent = h[PLS_DIVERGENT];
    s.placed = h[PLS_PLACED];
    s.votes = h[PLS_VOTES];
    s.columns = nbytes - n_ctgs;
    s.uncovered = h[PLS_UNCOVERED];
    s.thin = h[PLS_THIN];
    s.disputed = h[PLS_DISPUTED];
    s.confirmed = h[PLS_CONFIRMED];
    s.changed = h[PLS_CHANGED];
    s.filled = h[PLS_FILLED];
    s.sort_passes = (uint64_t)passes;
    *io.stats = s;
  }
  return KC_OK;
}

int kc_ctg_polish(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns,
                  uint64_t n_alns, int on_device, const kc_polish_params *p, uint8_t *out, uint16_t *counts, kc_polish_ctg *ctgs,
                  kc_polish_fix *fixes, uint64_t fix_capacity, kc_polish_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p) return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: params is NULL");
  if (p->edge_clip > KC_DEPTH_MAX_EDGE || (p->flags & ~KC_POLISH_BEST_ONLY))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: edge_clip %u over %d or unknown flags 0x%x", p->edge_clip, KC_DEPTH_MAX_EDGE, p->flags);
  if (!p->min_depth) return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: min_depth is 0, at least 1");
  if (p->min_permille > POLISH_MAX_PERMILLE)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: min_permille is %u, at most %u", p->min_permille, POLISH_MAX_PERMILLE);
  if (p->min_qual > POLISH_MAX_QUAL) return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: min_qual is %u, at most %u", p->min_qual, POLISH_MAX_QUAL);
  if (!c) return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: ctx is NULL");
  if (!out || (nreads && !offsets) || (n_alns && !alns))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: %s is NULL", !out ? "out" : (nreads && !offsets) ? "offsets" : "alns");
  if (on_device && (((uintptr_t)alns | (uintptr_t)ctgs | (uintptr_t)fixes) & 15)) return misaligned_records("kc_ctg_polish");
  if (on_device && ((((uintptr_t)offsets) & 7) || (((uintptr_t)counts) & 1)))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_polish: device offsets are 8-byte aligned, counts 2-byte");
  if (!c->ai_ready) return no_ctg_index("kc_ctg_polish");
  if (nreads > 0xFFFFFFFFull || n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_ctg_polish: %llu reads and %llu records, an index of either takes 32 bits", (unsigned long long)nreads,
                (unsigned long long)n_alns);
  const PolishIo io{bases, quals, offsets, nreads, alns, n_alns, on_device, out, counts, ctgs, fixes, fix_capacity, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return polish_run(c, b, io, *p); });
}
