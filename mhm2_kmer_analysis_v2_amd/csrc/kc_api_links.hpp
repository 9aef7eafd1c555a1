// kc_api_links.hpp -- kc_ctg_links (kernels in kc_links.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_lassm.hpp; the radix passes are kc_sort.hpp's.

static_assert(sizeof(kc_link_params) == 32 && sizeof(kc_ctg_link) == 48 && sizeof(kc_link_stats) == 128, "the header's layouts");
static_assert(KC_LINK_MAX_SLACK == LINK_MAX_SLACK && KC_LINK_MAX_OVERLAP == LINK_MAX_OVERLAP && KC_LINK_MAX_READ_ALNS == LINK_MAX_READ_ALNS,
              "the header's limits are the kernels'");
static_assert(KC_INSERT_MAX < LINK_GAP_BIAS && KC_LINK_MAX_OVERLAP < LINK_GAP_BIAS && 2 * LINK_GAP_BIAS <= LINK_SPAN,
              "a biased gap fits under the kind");

struct LinkIo {
  const uint64_t *offsets;
  uint64_t nreads;
  const kc_gap_aln *alns;
  uint64_t n_alns;
  const kc_pair_rec *pairs;
  int on_device;
  kc_ctg_link *links;
  uint64_t capacity;
  uint64_t *end_first, *n_links;
  kc_link_stats *stats;
};

static int links_run(kc_ctx *c, CallBufs &b, const LinkIo &io, const kc_link_params &p) {
  const uint64_t n_ctgs = c->ai.n_ctgs, n_ends = 2 * n_ctgs, nreads = io.nreads, n_alns = io.n_alns;
  const uint64_t npairs = io.pairs ? nreads / 2 : 0, units = nreads + npairs;
  const uint64_t rtiles = (nreads + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE, utiles = (units + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  const bool dev = io.on_device != 0;
  LinkArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  LassmArgs la;
  memset(&la, 0, sizeof(la));
  uint64_t *d_als;
  StagedIn<uint64_t> offs = staged_offsets(io.offsets, nreads, dev);
  StagedIn<uint4> alns{io.alns, dev, n_alns * sizeof(kc_gap_aln)}, pairs{io.pairs, dev, npairs * sizeof(kc_pair_rec)};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(LKS_COUNT);
    la.st = m.take<uint64_t>(LS_COUNT);
    d.st = m.take<uint64_t>(DPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    a.rfirst = m.take<uint64_t>(nreads);
    a.rbase = m.take<uint64_t>(rtiles);
    a.rcur = m.take<uint32_t>(nreads);
    zeroed = m.used;
    a.ufirst = m.take<uint64_t>(units);
    a.ubase = m.take<uint64_t>(utiles);
    offs.reserve(m);
    alns.reserve(m);
    pairs.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(alns.upload(c));
  KCTRY(pairs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(la.st + LS_BAD_PAIR, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  const dim3 tpb(256), stat_tpb(LINK_STAT_TPB);  // the kernels that count statistics: one atomic a workgroup and counter
  // ---- the checks: nothing is stored through the caller's pointers before the last of them has passed
  KCTRY(check_read_lengths(c, KT_LINK_LENGTHS, "kc_ctg_links", offs.d, nreads, d_als));
  KCTRY(check_read_records(c, d, KT_LINK_CHECK, "kc_ctg_links", alns.d, n_alns, offs.d, nreads));
  la.pairs = pairs.d;
  la.alns = alns.d;
  la.n_alns = n_alns;
  la.nreads = nreads;
  KCTRY(check_pairs(c, la, npairs, KT_LINK_PAIR_CHECK, "kc_ctg_links"));
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.alns = alns.d;
  a.n_alns = n_alns;
  a.offsets = offs.d;
  a.nreads = nreads;
  a.pairs = npairs ? pairs.d : nullptr;
  a.min_score = p.min_score;
  a.min_len = p.min_len;
  a.end_slack = p.end_slack;
  a.max_overlap = p.max_overlap;
  a.max_splint_gap = p.max_splint_gap;
  a.insert_avg = p.insert_avg;
  a.max_insert = p.max_insert;
  a.max_read_alns = p.max_read_alns;
  uint64_t h[LKS_COUNT];
  // ---- the passing records by read
  if (n_alns) {
    KCTRY(launch_timed(c, KT_LINK_GROUP_COUNT, kc_link_group_kernel<false>, blocks_for(n_alns, LINK_STAT_TPB), stat_tpb, 0, a));
    KCTRY(tiled_scan(c, KT_LINK_TILE_SCAN, KT_LINK_SCAN, a.rfirst, nreads, a.rbase, a.st + LKS_SLOT_TOTAL));
    KCTRY(read_back(c, h, a.st));
    if (h[LKS_SLOT_TOTAL]) {
      KCTRY(b.alloc(&a.info, h[LKS_SLOT_TOTAL] * sizeof(uint4)));
      KCTRY(launch_timed(c, KT_LINK_GROUP_FILL, kc_link_group_kernel<true>, blocks_for(n_alns), tpb, 0, a));
    }
  }
  // ---- candidates: count, scan, write
  if (units) {
    KCTRY(launch_timed(c, KT_LINK_CANDS_COUNT, kc_link_cands_kernel<false>, blocks_for(units, LINK_STAT_TPB), stat_tpb, 0, a));
    KCTRY(tiled_scan(c, KT_LINK_TILE_SCAN, KT_LINK_SCAN, a.ufirst, units, a.ubase, a.st + LKS_CAND_TOTAL));
  }
  KCTRY(read_back(c, h, a.st));
  const uint64_t n_cands = h[LKS_CAND_TOTAL], n = 2 * n_cands;  // every candidate is an item in either direction
  if (n_cands >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_ctg_links: %llu candidates, the sort's permutation holds fewer than 2^31", (unsigned long long)n_cands);
  const uint64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE, ncnt = ntiles * SORT_DIGITS, nheads = (n + LINK_TILE - 1) / LINK_TILE;
  uint64_t *kbuf[2] = {nullptr, nullptr}, *cnt = nullptr, *tile_heads = nullptr;
  uint32_t *ibuf[2] = {nullptr, nullptr};
  int cur = 0;
  uint64_t n_runs = 0;
  if (n) {
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      kbuf[0] = m.take<uint64_t>(n);
      kbuf[1] = m.take<uint64_t>(n);
      ibuf[0] = m.take<uint32_t>(n);
      ibuf[1] = m.take<uint32_t>(n);
      a.payload = m.take<uint32_t>(n_cands);
      cnt = m.take<uint64_t>(ncnt);
      tile_heads = m.take<uint64_t>(nheads);
      return m.used;
    }));
    a.keys = kbuf[0];
    KCTRY(launch_timed(c, KT_LINK_CANDS_WRITE, kc_link_cands_kernel<true>, blocks_for(units), tpb, 0, a));
    // ---- order the items by (from, to): only the bits an end's number has, `to` in the low word, `from` in the high
    const int bits = 64 - __builtin_clzll((unsigned long long)(n_ends - 1) | 1ull);
    const uint32_t *perm = nullptr;  // the identity until the first pass has run
    for (int base = 0; base < 64; base += 32)
      for (int s = 0; s < bits; s += SORT_BITS) {
        const int shift = base + s;
        const uint32_t mask = (1u << std::min(SORT_BITS, bits - s)) - 1u;
        KCTRY(launch_timed(c, KT_LINK_SORT_HIST, kc_sort_hist_kernel<false>, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)nullptr, 1,
                           0, perm, kbuf[cur], n, ntiles, shift, mask, cnt));
        KCTRY(launch_timed(c, KT_LINK_SORT_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{cnt}}, ncnt, a.st + LKS_SORT_TOTAL));
        KCTRY(launch_timed(c, KT_LINK_SORT_SCATTER, kc_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)kbuf[cur],
                           perm, kbuf[cur ^ 1], ibuf[cur ^ 1], n, ntiles, shift, mask, (const uint64_t *)cnt));
        cur ^= 1;
        perm = ibuf[cur];
      }
    // ---- runs of equal keys are the directed records
    KCTRY(launch_timed(c, KT_LINK_HEADS, kc_link_heads_kernel, dim3((unsigned)nheads), dim3(LINK_TILE), 0, (const uint64_t *)kbuf[cur], n,
                       tile_heads));
    KCTRY(launch_timed(c, KT_LINK_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{tile_heads}}, nheads, a.st + LKS_RUN_TOTAL));
    KCTRY(read_back(c, &n_runs, a.st + LKS_RUN_TOTAL, 1));
  }
  const bool fits = io.links && io.capacity >= n_runs;
  LinkAcc acc;
  memset(&acc, 0, sizeof(acc));
  StagedOut<uint4> links{io.links, dev, n_runs * sizeof(kc_ctg_link)};
  StagedOut<uint64_t> ef{io.end_first, dev, (n_ends + 1) * 8};
  size_t acc_zeroed = 0, acc_min = 0, acc_max = 0;
  KCTRY(b.carve([&](uint8_t *base) {  // nothing at all where there are no runs and nothing to copy out
    Carver m{base, 0};
    acc.cnt = m.take<uint64_t>(n_runs);
    acc.ssum = m.take<uint64_t>(n_runs);
    acc.psum = m.take<uint64_t>(n_runs);
    acc_zeroed = m.used;
    acc.smin = m.take<int32_t>(n_runs);
    acc.pmin = m.take<int32_t>(n_runs);
    acc_min = m.used;
    acc.smax = m.take<int32_t>(n_runs);
    acc.pmax = m.take<int32_t>(n_runs);
    acc_max = m.used;
    acc.key = m.take<uint64_t>(n_runs);
    links.reserve(m, fits);
    ef.reserve(m, fits);
    return m.used;
  }));
  if (n_runs) {
    HIPCHK(hipMemsetAsync(acc.cnt, 0, acc_zeroed, c->stream));
    HIPCHK(hipMemsetAsync(acc.smin, 0x7F, acc_min - acc_zeroed, c->stream));
    HIPCHK(hipMemsetAsync(acc.smax, 0x80, acc_max - acc_min, c->stream));
    KCTRY(launch_timed(c, KT_LINK_REDUCE, kc_link_reduce_kernel, dim3((unsigned)nheads), dim3(LINK_TILE), 0, (const uint64_t *)kbuf[cur],
                       (const uint32_t *)ibuf[cur], (const uint32_t *)a.payload, n, (const uint64_t *)tile_heads, acc));
    KCTRY(launch_timed(c, KT_LINK_EMIT, kc_link_emit_kernel, blocks_for(n_runs, LINK_STAT_TPB), stat_tpb, 0, acc, n_runs, links.d, a.st));
  }
  if (ef.d)
    KCTRY(launch_timed(c, KT_LINK_END_FIRST, kc_link_end_first_kernel, blocks_for(n_ends + 1), tpb, 0, (const uint64_t *)acc.key, n_runs, n_ends, ef.d));
  KCTRY(links.download(c));
  KCTRY(ef.download(c));
  KCTRY(read_back(c, h, a.st));
  *io.n_links = n_runs;
  if (io.stats) {
    kc_link_stats st;
    memset(&st, 0, sizeof(st));
    st.reads = nreads;
    st.reads_over_cap = h[LKS_OVER_CAP];
    st.records = n_alns;
    st.none = h[LKS_NONE];
    st.filtered = h[LKS_FILTERED];
    st.passed = h[LKS_PASSED];
    st.splint_cands = h[LKS_SPLINT_CANDS];
    st.splints_gap_out = h[LKS_GAP_OUT];
    st.span_cands = h[LKS_SPAN_CANDS];
    st.spans_too_far = h[LKS_TOO_FAR];
    st.links = h[LKS_LINKS];
    st.links_splint_only = h[LKS_SPLINT_ONLY];
    st.links_span_only = h[LKS_SPAN_ONLY];
    st.links_both = h[LKS_BOTH];
    st.ends_linked = h[LKS_ENDS];
    *io.stats = st;
  }
  if (io.links && !fits)
    return fail(KC_ERR_CAPACITY, "kc_ctg_links: %llu records, the array holds %llu", (unsigned long long)n_runs, (unsigned long long)io.capacity);
  return KC_OK;
}

extern "C" int kc_ctg_links(kc_ctx *c, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs,
                            int on_device, const kc_link_params *p, kc_ctg_link *links, uint64_t capacity, uint64_t *end_first, uint64_t *n_links,
                            kc_link_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_links) return KC_ERR_INVALID_ARG;
  if (p->end_slack > KC_LINK_MAX_SLACK) return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: end_slack %u over %d", p->end_slack, KC_LINK_MAX_SLACK);
  if (p->max_overlap > KC_LINK_MAX_OVERLAP || p->max_splint_gap > KC_LINK_MAX_SLACK)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: max_overlap %u over %d or max_splint_gap %u over %d", p->max_overlap, KC_LINK_MAX_OVERLAP,
                p->max_splint_gap, KC_LINK_MAX_SLACK);
  if (p->insert_avg < 1 || p->insert_avg > p->max_insert || p->max_insert > KC_INSERT_MAX)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: insert_avg %u, max_insert %u outside 1 <= insert_avg <= max_insert <= %d", p->insert_avg,
                p->max_insert, KC_INSERT_MAX);
  if (p->max_read_alns < 2 || p->max_read_alns > KC_LINK_MAX_READ_ALNS)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: max_read_alns %u outside 2 .. %d", (unsigned)p->max_read_alns, KC_LINK_MAX_READ_ALNS);
  if (p->flags) return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: unknown flags 0x%x", (unsigned)p->flags);
  if (nreads & 1)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: %llu reads are no pairs (reads 2p and 2p + 1 are mates)", (unsigned long long)nreads);
  if (!c || (nreads && !offsets) || (n_alns && !alns) || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs | (uintptr_t)links) & 15)) return misaligned_records("kc_ctg_links");
  if (on_device && (((uintptr_t)offsets | (uintptr_t)end_first) & 7))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_links: device offsets and end_first are 8-byte aligned");
  if (!c->ai_ready) return no_ctg_index("kc_ctg_links");
  if (n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_ctg_links: %llu records, a pair holds a record's index in 32 bits", (unsigned long long)n_alns);
  const LinkIo io{offsets, nreads, alns, n_alns, pairs, on_device, links, capacity, end_first, n_links, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return links_run(c, b, io, *p); });
}
