// kc_api_links.hpp -- kc_ctg_links (kernels in kc_links.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_lassm.hpp, whose pair check and buffers it uses; the record check is kc_api_depth.hpp's, the length check
// kc_api_align.hpp's, the radix passes kc_sort.hpp's.

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

static int links_run(kc_ctx *c, LassmBufs &b, const LinkIo &io, const kc_link_params &p) {
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
  uint64_t *d_als, *d_offs = nullptr;
  uint4 *d_alns = nullptr, *d_pairs = nullptr;
  size_t zeroed = 0;
  auto layout = [&](uint8_t *base) {
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
    if (!dev) {
      d_offs = m.take<uint64_t>(nreads + 1);
      d_alns = m.take<uint4>(2 * n_alns);
      d_pairs = m.take<uint4>(npairs);
    }
    return m.used;
  };
  HIPCHK(hipMalloc((void **)&b.p[0], layout(nullptr)));
  layout(b.p[0]);
  if (dev) {
    d_offs = const_cast<uint64_t *>(io.offsets);
    d_alns = (uint4 *)const_cast<kc_gap_aln *>(io.alns);
    d_pairs = (uint4 *)const_cast<kc_pair_rec *>(io.pairs);
  } else {
    if (nreads) HIPCHK(hipMemcpyAsync(d_offs, io.offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_alns) HIPCHK(hipMemcpyAsync(d_alns, io.alns, n_alns * sizeof(kc_gap_aln), hipMemcpyHostToDevice, c->stream));
    if (npairs) HIPCHK(hipMemcpyAsync(d_pairs, io.pairs, npairs * sizeof(kc_pair_rec), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(la.st + LS_BAD_PAIR, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d_als + ALS_BAD_READ, 0xFF, 8, c->stream));
  auto blocks = [](uint64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  const dim3 tpb(256), stat_tpb(LINK_STAT_TPB);  // the kernels that count statistics: one atomic a workgroup and counter
  auto stat_blocks = [](uint64_t n) { return dim3((unsigned)((n + LINK_STAT_TPB - 1) / LINK_STAT_TPB)); };
  // ---- the checks: nothing is stored through the caller's pointers before the last of them has passed
  if (nreads) {
    KCTRY(launch_timed(c, KT_LINK_LENGTHS, kc_align_lengths_kernel, blocks(nreads), tpb, 0, (const uint64_t *)d_offs, nreads, d_als));
    uint64_t bad_read = ~0ull;
    HIPCHK(hipMemcpyAsync(&bad_read, d_als + ALS_BAD_READ, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad_read != ~0ull) {
      snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: read %llu is longer than %d bases, or its offsets decrease",
               (unsigned long long)bad_read, KC_ALIGN_MAX_READ_LEN);
      return KC_ERR_INVALID_ARG;
    }
  }
  d.offs = c->ai.offs;
  d.n_ctgs = (uint32_t)n_ctgs;
  d.nbytes = (uint32_t)c->ai_nbytes;
  d.alns = d_alns;
  d.n_alns = n_alns;
  d.nreads = nreads;
  d.offsets = d_offs;
  KCTRY(depth_check(c, d, KT_LINK_CHECK, 1, "kc_ctg_links"));
  if (npairs) {
    la.pairs = d_pairs;
    la.alns = d_alns;
    la.n_alns = n_alns;
    la.nreads = nreads;
    KCTRY(launch_timed(c, KT_LINK_PAIR_CHECK, kc_lassm_pair_check_kernel, blocks(npairs), tpb, 0, la));
    uint64_t bad = ~0ull;
    HIPCHK(hipMemcpyAsync(&bad, la.st + LS_BAD_PAIR, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad != ~0ull) {
      snprintf(g_last_error, sizeof(g_last_error),
               "kc_ctg_links: pair %llu names a record that is out of range, of another read or of kind KC_GAP_NONE", (unsigned long long)bad);
      return KC_ERR_INVALID_ARG;
    }
  }
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.alns = d_alns;
  a.n_alns = n_alns;
  a.offsets = d_offs;
  a.nreads = nreads;
  a.pairs = npairs ? d_pairs : nullptr;
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
    KCTRY(launch_timed(c, KT_LINK_GROUP_COUNT, kc_link_group_kernel<false>, stat_blocks(n_alns), stat_tpb, 0, a));
    KCTRY(launch_timed(c, KT_LINK_TILE_SCAN, kc_link_tile_scan_kernel, dim3((unsigned)rtiles), dim3(LINK_TILE), 0, a.rfirst, nreads, a.rbase));
    KCTRY(launch_timed(c, KT_LINK_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.rbase}}, rtiles, a.st + LKS_SLOT_TOTAL));
    HIPCHK(hipMemcpyAsync(h, a.st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h[LKS_SLOT_TOTAL]) {
      HIPCHK(hipMalloc((void **)&b.p[1], h[LKS_SLOT_TOTAL] * sizeof(uint4)));
      a.info = (uint4 *)b.p[1];
      KCTRY(launch_timed(c, KT_LINK_GROUP_FILL, kc_link_group_kernel<true>, blocks(n_alns), tpb, 0, a));
    }
  }
  // ---- candidates: count, scan, write
  if (units) {
    KCTRY(launch_timed(c, KT_LINK_CANDS_COUNT, kc_link_cands_kernel<false>, stat_blocks(units), stat_tpb, 0, a));
    KCTRY(launch_timed(c, KT_LINK_TILE_SCAN, kc_link_tile_scan_kernel, dim3((unsigned)utiles), dim3(LINK_TILE), 0, a.ufirst, units, a.ubase));
    KCTRY(launch_timed(c, KT_LINK_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.ubase}}, utiles, a.st + LKS_CAND_TOTAL));
  }
  HIPCHK(hipMemcpyAsync(h, a.st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t n_cands = h[LKS_CAND_TOTAL], n = 2 * n_cands;  // every candidate is an item in either direction
  if (n_cands >= (1ull << 31)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: %llu candidates, the sort's permutation holds fewer than 2^31",
             (unsigned long long)n_cands);
    return KC_ERR_CAPACITY;
  }
  const uint64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE, ncnt = ntiles * SORT_DIGITS, nheads = (n + LINK_TILE - 1) / LINK_TILE;
  uint64_t *kbuf[2] = {nullptr, nullptr}, *cnt = nullptr, *tile_heads = nullptr;
  uint32_t *ibuf[2] = {nullptr, nullptr};
  int cur = 0;
  uint64_t n_runs = 0;
  if (n) {
    auto work = [&](uint8_t *base) {
      Carver m{base, 0};
      kbuf[0] = m.take<uint64_t>(n);
      kbuf[1] = m.take<uint64_t>(n);
      ibuf[0] = m.take<uint32_t>(n);
      ibuf[1] = m.take<uint32_t>(n);
      a.payload = m.take<uint32_t>(n_cands);
      cnt = m.take<uint64_t>(ncnt);
      tile_heads = m.take<uint64_t>(nheads);
      return m.used;
    };
    HIPCHK(hipMalloc((void **)&b.p[2], work(nullptr)));
    work(b.p[2]);
    a.keys = kbuf[0];
    KCTRY(launch_timed(c, KT_LINK_CANDS_WRITE, kc_link_cands_kernel<true>, blocks(units), tpb, 0, a));
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
    HIPCHK(hipMemcpyAsync(&n_runs, a.st + LKS_RUN_TOTAL, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  const bool fits = io.links && io.capacity >= n_runs;
  LinkAcc acc;
  memset(&acc, 0, sizeof(acc));
  uint4 *d_links = nullptr;
  uint64_t *d_ef = nullptr;
  size_t acc_zeroed = 0, acc_min = 0, acc_max = 0;
  auto fold = [&](uint8_t *base) {
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
    if (!dev && fits) {
      d_links = m.take<uint4>(3 * n_runs);
      if (io.end_first) d_ef = m.take<uint64_t>(n_ends + 1);
    }
    return m.used;
  };
  if (fold(nullptr)) {
    HIPCHK(hipMalloc((void **)&b.p[3], fold(nullptr)));
    fold(b.p[3]);
  }
  if (dev && fits) {
    d_links = (uint4 *)io.links;
    d_ef = io.end_first;
  }
  if (n_runs) {
    HIPCHK(hipMemsetAsync(acc.cnt, 0, acc_zeroed, c->stream));
    HIPCHK(hipMemsetAsync(acc.smin, 0x7F, acc_min - acc_zeroed, c->stream));
    HIPCHK(hipMemsetAsync(acc.smax, 0x80, acc_max - acc_min, c->stream));
    KCTRY(launch_timed(c, KT_LINK_REDUCE, kc_link_reduce_kernel, dim3((unsigned)nheads), dim3(LINK_TILE), 0, (const uint64_t *)kbuf[cur],
                       (const uint32_t *)ibuf[cur], (const uint32_t *)a.payload, n, (const uint64_t *)tile_heads, acc));
    KCTRY(launch_timed(c, KT_LINK_EMIT, kc_link_emit_kernel, stat_blocks(n_runs), stat_tpb, 0, acc, n_runs, d_links, a.st));
  }
  if (fits && d_ef)
    KCTRY(launch_timed(c, KT_LINK_END_FIRST, kc_link_end_first_kernel, blocks(n_ends + 1), tpb, 0, (const uint64_t *)acc.key, n_runs, n_ends, d_ef));
  HIPCHK(hipMemcpyAsync(h, a.st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  if (!dev && fits) {
    if (n_runs) HIPCHK(hipMemcpyAsync(io.links, d_links, n_runs * sizeof(kc_ctg_link), hipMemcpyDeviceToHost, c->stream));
    if (d_ef) HIPCHK(hipMemcpyAsync(io.end_first, d_ef, (n_ends + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
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
  if (io.links && !fits) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: %llu records, the array holds %llu", (unsigned long long)n_runs,
             (unsigned long long)io.capacity);
    return KC_ERR_CAPACITY;
  }
  return KC_OK;
}

extern "C" int kc_ctg_links(kc_ctx *c, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs,
                            int on_device, const kc_link_params *p, kc_ctg_link *links, uint64_t capacity, uint64_t *end_first, uint64_t *n_links,
                            kc_link_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_links) return KC_ERR_INVALID_ARG;
  if (p->end_slack > KC_LINK_MAX_SLACK) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: end_slack %u over %d", p->end_slack, KC_LINK_MAX_SLACK);
    return KC_ERR_INVALID_ARG;
  }
  if (p->max_overlap > KC_LINK_MAX_OVERLAP || p->max_splint_gap > KC_LINK_MAX_SLACK) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: max_overlap %u over %d or max_splint_gap %u over %d", p->max_overlap,
             KC_LINK_MAX_OVERLAP, p->max_splint_gap, KC_LINK_MAX_SLACK);
    return KC_ERR_INVALID_ARG;
  }
  if (p->insert_avg < 1 || p->insert_avg > p->max_insert || p->max_insert > KC_INSERT_MAX) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: insert_avg %u, max_insert %u outside 1 <= insert_avg <= max_insert <= %d",
             p->insert_avg, p->max_insert, KC_INSERT_MAX);
    return KC_ERR_INVALID_ARG;
  }
  if (p->max_read_alns < 2 || p->max_read_alns > KC_LINK_MAX_READ_ALNS) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: max_read_alns %u outside 2 .. %d", (unsigned)p->max_read_alns,
             KC_LINK_MAX_READ_ALNS);
    return KC_ERR_INVALID_ARG;
  }
  if (p->flags) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: unknown flags 0x%x", (unsigned)p->flags);
    return KC_ERR_INVALID_ARG;
  }
  if (nreads & 1) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: %llu reads are no pairs (reads 2p and 2p + 1 are mates)",
             (unsigned long long)nreads);
    return KC_ERR_INVALID_ARG;
  }
  if (!c || (nreads && !offsets) || (n_alns && !alns) || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs | (uintptr_t)links) & 15)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: a device record array is 16-byte aligned");
    return KC_ERR_INVALID_ARG;
  }
  if (on_device && (((uintptr_t)offsets | (uintptr_t)end_first) & 7)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: device offsets and end_first are 8-byte aligned");
    return KC_ERR_INVALID_ARG;
  }
  if (!c->ai_ready) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: no contig index (kc_ctg_index_build)");
    return KC_ERR_STATE;
  }
  if (n_alns > 0xFFFFFFFFull) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_ctg_links: %llu records, a pair holds a record's index in 32 bits", (unsigned long long)n_alns);
    return KC_ERR_CAPACITY;
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  LassmBufs b;
  const LinkIo io{offsets, nreads, alns, n_alns, pairs, on_device, links, capacity, end_first, n_links, stats};
  const int rc = links_run(c, b, io, *p);
  if (rc) (void)hipStreamSynchronize(c->stream);
  b.release();
  return rc;
}
