// kc_api_unitig.hpp -- kc_build_unitigs (kernels in kc_unitig.hpp).  Part of kc_api.hip's translation unit, like
// kc_api_sort.hpp.

// rounds of pointer jumping after which a path of up to 2n nodes has been walked: ceil(log2 2n) + 1
static int unitig_rounds(uint64_t n) {
  int r = 0;
  while ((1ull << r) < 2 * n) r++;
  return r + 1;
}

template <int NL>
static int unitig_run(kc_ctx *c, CallBufs &b, uint8_t *d_seqs, uint64_t capacity, uint16_t *d_depths, uint64_t *d_offsets,
                      uint64_t unitigs_capacity, uint64_t *d_kmer_sums, uint64_t *n_unitigs, uint64_t *nbytes, kc_unitig_stats *stats) {
  KCTRY(ensure_index<NL>(c));
  const uint32_t n = (uint32_t)c->out_n, nn = 2 * n;
  uint32_t *next;
  uint2 *jump[3];
  uint64_t *size, *num, *st;
  uint8_t *sel;
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    next = m.take<uint32_t>(nn);
    for (auto &j : jump) j = m.take<uint2>(nn);
    size = m.take<uint64_t>(n);
    num = m.take<uint64_t>(n);
    sel = m.take<uint8_t>(n);
    st = m.take<uint64_t>(UST_COUNT);
    return m.used;
  };
  KCTRY(b.carve(layout));
  // size .. st are neighbours in the layout
  HIPCHK(hipMemsetAsync(size, 0, (size_t)((uint8_t *)(st + UST_COUNT) - (uint8_t *)size), c->stream));
  const dim3 per_result = blocks_for(n, UNITIG_TPB), per_node = blocks_for(nn, UNITIG_TPB), tpb(UNITIG_TPB);
  const int rounds = unitig_rounds(n);
  KCTRY(launch_timed(c, KT_UNITIG_LINKS, kc_unitig_links_kernel<NL>, per_result, tpb, 0, (const uint64_t *)c->d_out_keys,
                     (const uint8_t *)c->d_out_left, (const uint8_t *)c->d_out_right, n, c->k, (const uint32_t *)c->d_index, c->index_cap - 1,
                     (uint2 *)next, (uint4 *)jump[0]));
  int cur = 0;  // the cycle search goes between jump[0] and jump[1] ...
  for (int r = 0; r < rounds; r++, cur ^= 1)
    KCTRY(launch_timed(c, KT_UNITIG_MIN_JUMP, kc_unitig_min_jump_kernel, per_node, tpb, 0, (const uint2 *)jump[cur], jump[cur ^ 1], nn));
  KCTRY(launch_timed(c, KT_UNITIG_CUT, kc_unitig_cut_kernel, per_result, tpb, 0, (const uint4 *)jump[cur], (uint2 *)next, (uint4 *)jump[2], n, st));
  int from = 2, to = cur ^ 1;  // ... the ranking starts in jump[2] and goes between it and the buffer the search left free
  for (int r = 0; r < rounds; r++, std::swap(from, to))
    KCTRY(launch_timed(c, KT_UNITIG_RANK_JUMP, kc_unitig_rank_jump_kernel, per_node, tpb, 0, (const uint2 *)jump[from], jump[to], nn));
  const uint2 *rank = jump[from];
  KCTRY(launch_timed(c, KT_UNITIG_SELECT, kc_unitig_select_kernel, per_node, tpb, 0, rank, (const uint32_t *)next, nn, c->k, size, num, sel, st));
  KCTRY(launch_timed(c, KT_UNITIG_SCAN, kc_scan_kernel<2>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<2>{{size, num}}, (uint64_t)n, st + UST_TOTALS));
  uint64_t h[UST_COUNT];
  KCTRY(read_back(c, h, st));
  const uint64_t total = h[UST_TOTALS], nu = h[UST_TOTALS + 1];
  *nbytes = total;
  *n_unitigs = nu;
  if (stats) {
    stats->kmers = n;
    stats->unitigs = nu;
    stats->singletons = h[UST_SINGLETONS];
    stats->circular = h[UST_CIRCULAR];
    stats->bases = total - nu;
    stats->longest = h[UST_LONGEST];
  }
  if (!d_seqs || !d_offsets) return KC_OK;  // a size query
  if (total > capacity || nu > unitigs_capacity)
    return fail(KC_ERR_CAPACITY, "kc_build_unitigs: %llu unitigs are %llu bytes, the arrays hold %llu and %llu", (unsigned long long)nu,
                (unsigned long long)total, (unsigned long long)unitigs_capacity, (unsigned long long)capacity);
  uint64_t *sums = d_kmer_sums;
  if (!sums && d_depths) KCTRY(b.alloc(&sums, nu * 8));  // the caller keeps none
  if (sums) HIPCHK(hipMemsetAsync(sums, 0, nu * 8, c->stream));
  KCTRY(launch_timed(c, KT_UNITIG_WRITE, kc_unitig_write_kernel, per_node, tpb, 0, rank, (const uint32_t *)next, (const uint64_t *)c->d_out_keys,
                     c->nl, (const uint16_t *)c->d_out_counts, (const uint8_t *)sel, (const uint64_t *)size, (const uint64_t *)num, nn, c->k, total,
                     nu, d_seqs, d_offsets, sums));
  if (d_depths)
    KCTRY(launch_timed(c, KT_UNITIG_DEPTH, kc_unitig_depth_kernel, per_node, tpb, 0, rank, (const uint32_t *)next, (const uint8_t *)sel,
                       (const uint64_t *)size, (const uint64_t *)num, (const uint64_t *)d_offsets, (const uint64_t *)sums, nn, c->k, total,
                       d_depths));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

extern "C" int kc_build_unitigs(kc_ctx *c, uint8_t *d_seqs, uint64_t capacity, uint16_t *d_depths, uint64_t *d_offsets, uint64_t unitigs_capacity,
                                uint64_t *d_kmer_sums, uint64_t *n_unitigs, uint64_t *nbytes, kc_unitig_stats *stats) {
  if (!c || !n_unitigs || !nbytes) return KC_ERR_INVALID_ARG;
  *n_unitigs = *nbytes = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!c->finalized) return KC_ERR_STATE;
  if (c->cfg.rank_n > 1)
    return fail(KC_ERR_STATE, "kc_build_unitigs: this context is one of %d ranks, and links across shards are not followed", c->cfg.rank_n);
  if (c->out_n >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_build_unitigs: %llu results, oriented node ids are 32-bit (fewer than 2^31 results)",
                (unsigned long long)c->out_n);
  if (!c->out_n) {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (d_seqs && d_offsets) {
      HIPCHK(hipMemsetAsync(d_offsets, 0, 8, c->stream));  // offsets[0] = 0: the one entry of no unitigs
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return KC_OK;
  }
  KCTRY(kc_sort_results(c, nullptr));  // result order is key order from here on
  return call_with_bufs(c, [&](CallBufs &b) {
    return with_nl(c, [&](auto nl) {
      return unitig_run<nl>(c, b, d_seqs, capacity, d_depths, d_offsets, unitigs_capacity, d_kmer_sums, n_unitigs, nbytes, stats);
    });
  });
}
