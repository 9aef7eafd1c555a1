// kc_api_shuffle.hpp -- kc_shuffle_reads (kernels in kc_shuffle.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_close.hpp; the radix passes are kc_sort.hpp's, the scan kc_api_call.hpp's.

static_assert(sizeof(kc_shuffle_stats) == 80, "the header's layout");
static_assert(KC_SHUFFLE_MAX_PARTS == SHUF_MAX_PARTS && KC_SHUFFLE_NO_HOME == SHUF_NO_HOME, "the header's limits are the kernels'");

struct ShufIo {
  const uint8_t *bases, *quals;
  const uint64_t *offsets;
  uint64_t nreads;
  const kc_gap_aln *alns;
  uint64_t n_alns;
  const kc_pair_rec *pairs;
  int on_device;
  uint32_t parts;
  uint8_t *bases_out, *quals_out;
  uint64_t *offsets_out;
  uint32_t *order, *home;
  uint64_t *part_starts;
  kc_gap_aln *alns_out;
  kc_pair_rec *pairs_out;
  kc_shuffle_stats *stats;
};

static int shuffle_run(kc_ctx *c, CallBufs &b, const ShufIo &io) {
  const uint64_t nreads = io.nreads, npairs = nreads / 2, n_alns = io.n_alns, parts = io.parts;
  const uint64_t rtiles = (nreads + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  const uint64_t ntiles = (npairs + SORT_TILE - 1) / SORT_TILE, ncnt = ntiles * SORT_DIGITS;
  const bool dev = io.on_device != 0;
  ShufArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  LassmArgs la;
  memset(&la, 0, sizeof(la));
  uint64_t *d_als, *kbuf[2] = {nullptr, nullptr}, *cnt = nullptr;
  uint32_t *ibuf[2] = {nullptr, nullptr};
  StagedIn<uint64_t> offs = staged_offsets(io.offsets, nreads, dev);
  StagedIn<uint4> alns{io.alns, dev, n_alns * sizeof(kc_gap_aln)}, pairs{io.pairs, dev, npairs * sizeof(kc_pair_rec)};
  StagedOut<uint64_t> offs_out{io.offsets_out, dev, (nreads + 1) * 8}, starts{io.part_starts, dev, (parts + 1) * 8};
  StagedOut<uint32_t> order{io.order, dev, npairs * 4}, home{io.home, dev, npairs * 4};
  StagedOut<uint4> alns_out{io.alns_out, dev, n_alns * sizeof(kc_gap_aln)}, pairs_out{io.pairs_out, dev, npairs * sizeof(kc_pair_rec)};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(SHS_COUNT);
    la.st = m.take<uint64_t>(LS_COUNT);
    d.st = m.take<uint64_t>(DPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    zeroed = m.used;
    kbuf[0] = m.take<uint64_t>(npairs);
    kbuf[1] = m.take<uint64_t>(npairs);
    ibuf[0] = m.take<uint32_t>(npairs);
    ibuf[1] = m.take<uint32_t>(npairs);
    cnt = m.take<uint64_t>(ncnt);
    a.lens = m.take<uint64_t>(nreads);
    a.lbase = m.take<uint64_t>(rtiles);
    a.psrc = m.take<uint64_t>(npairs);
    a.inv = m.take<uint32_t>(npairs);
    offs.reserve(m);
    alns.reserve(m);
    pairs.reserve(m);
    offs_out.reserve(m);
    starts.reserve(m);
    order.reserve(m);
    home.reserve(m);
    alns_out.reserve(m, n_alns != 0);
    pairs_out.reserve(m, npairs != 0);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(alns.upload(c));
  KCTRY(pairs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(la.st + LS_BAD_PAIR, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  // ---- the checks: nothing is stored through the caller's pointers before the last of them has passed
  uint64_t last = 0;
  KCTRY(check_read_lengths(c, KT_SHUF_LENGTHS, "kc_shuffle_reads", offs.d, nreads, d_als, nullptr, &last));
  KCTRY(check_read_records(c, d, KT_SHUF_CHECK, "kc_shuffle_reads", alns.d, n_alns, offs.d, nreads));
  la.pairs = pairs.d;
  la.alns = alns.d;
  la.n_alns = n_alns;
  la.nreads = nreads;
  KCTRY(check_pairs(c, la, npairs, KT_SHUF_PAIR_CHECK, "kc_shuffle_reads"));
  if (last && !io.bases) return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: bases is NULL and the reads have %llu bytes", (unsigned long long)last);
  // ---- the reads' bytes, in and out: a host caller's get room now that the lengths are known
  const uint8_t *d_bases = io.bases, *d_quals = io.quals;
  uint8_t *d_bases_out = io.bases_out, *d_quals_out = io.quals_out;
  KCTRY(b.alloc(&a.blk, ((last + (1ull << SHUF_BLOCK_SHIFT) - 1) >> SHUF_BLOCK_SHIFT) * 4));
  if (!dev && last) {
    KCTRY(b.alloc(&d_bases_out, last));
    if (io.quals) KCTRY(b.alloc(&d_quals_out, last));
    KCTRY(upload_reads(c, b, io.bases, last, &d_bases));
    if (io.quals) KCTRY(upload_reads(c, b, io.quals, last, &d_quals));
  }
  const uint32_t n_ctgs = c->ai.n_ctgs;
  const dim3 tpb(SHUF_TPB);
  uint64_t h[SHS_COUNT];
  memset(h, 0, sizeof(h));
  a.offs = c->ai.offs;
  a.n_ctgs = n_ctgs;
  a.parts = io.parts;
  a.alns = alns.d;
  a.n_alns = n_alns;
  a.pairs = pairs.d;
  a.npairs = npairs;
  a.offsets = offs.d;
  a.offsets_out = offs_out.d;
  a.part_starts = starts.d;
  a.order = order.d;
  a.home = home.d;
  a.alns_out = alns_out.d;
  a.pairs_out = pairs_out.d;
  int bits = 0;
  if (npairs) {
    // ---- the key: home << abits | anchor, abits the bits of the longest contig
    if (n_ctgs) KCTRY(launch_timed(c, KT_SHUF_LONGEST, kc_shuf_longest_kernel, blocks_for(n_ctgs, SHUF_TPB), tpb, 0, a.offs, n_ctgs, a.st));
    KCTRY(read_back(c, &h[SHS_LONGEST], a.st + SHS_LONGEST, 1));
    a.abits = (uint32_t)(64 - __builtin_clzll((unsigned long long)h[SHS_LONGEST] | 1ull)) - (h[SHS_LONGEST] ? 0u : 1u);
    bits = (int)a.abits + (n_ctgs ? 64 - __builtin_clzll((unsigned long long)n_ctgs) : 0);
    a.keys = kbuf[0];
    KCTRY(launch_timed(c, KT_SHUF_KEY, kc_shuf_key_kernel, blocks_for(npairs, LINK_STAT_TPB), dim3(LINK_STAT_TPB), 0, a));
    // ---- one stable sort of the permutation over the key's significant bits
    int cur = 0;
    const uint32_t *perm = nullptr;  // the identity until the first pass has run
    for (int shift = 0; shift < bits; shift += SORT_BITS) {
      const uint32_t mask = (1u << std::min(SORT_BITS, bits - shift)) - 1u;
      KCTRY(launch_timed(c, KT_SHUF_SORT_HIST, kc_sort_hist_kernel<false>, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)nullptr, 1, 0,
                         perm, kbuf[cur], npairs, ntiles, shift, mask, cnt));
      KCTRY(launch_timed(c, KT_SHUF_SORT_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{cnt}}, ncnt, a.st + SHS_SORT_TOTAL));
      KCTRY(launch_timed(c, KT_SHUF_SORT_SCATTER, kc_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(SORT_TPB), 0, (const uint64_t *)kbuf[cur], perm,
                         kbuf[cur ^ 1], ibuf[cur ^ 1], npairs, ntiles, shift, mask, (const uint64_t *)cnt));
      cur ^= 1;
      perm = ibuf[cur];
    }
    a.keys = kbuf[cur];
    a.perm = perm;
    // ---- the new order, the new offsets
    KCTRY(launch_timed(c, KT_SHUF_PLACE, kc_shuf_place_kernel, blocks_for(npairs, SHUF_TPB), tpb, 0, a));
    KCTRY(tiled_scan(c, KT_SHUF_TILE_SCAN, KT_SHUF_SCAN, a.lens, nreads, a.lbase, a.st + SHS_BYTES));
  }
  KCTRY(launch_timed(c, KT_SHUF_OFFSETS, kc_shuf_offsets_kernel, blocks_for(nreads + 1, SHUF_TPB), tpb, 0, a));
  // ---- the bytes
  if (last) {
    ShufCopy g;
    memset(&g, 0, sizeof(g));
    g.src[0] = d_bases;
    g.dst[0] = d_bases_out;
    g.src[1] = d_quals;
    g.dst[1] = d_quals_out;
    g.noff = offs_out.d;
    g.psrc = a.psrc;
    g.blk = a.blk;
    g.npairs = npairs;
    g.total = last;
    const uint64_t chunks = (last + 15 + 15) / 16;  // a misaligned array's first chunk is partial
    KCTRY(launch_timed(c, KT_SHUF_GATHER, kc_shuf_gather_kernel, dim3((unsigned)((chunks + SHUF_TPB - 1) / SHUF_TPB), d_quals ? 2u : 1u), tpb, 0, g));
  }
  if ((alns_out.d && n_alns) || (pairs_out.d && npairs))
    KCTRY(launch_timed(c, KT_SHUF_REMAP, kc_shuf_remap_kernel, blocks_for((alns_out.d ? n_alns : 0) + (pairs_out.d ? npairs : 0), SHUF_TPB), tpb, 0, a));
  KCTRY(launch_timed(c, KT_SHUF_PARTS, kc_shuf_parts_kernel, blocks_for(parts + 1, SHUF_TPB), tpb, 0, a));
  if (!dev && last) {
    HIPCHK(hipMemcpyAsync(io.bases_out, d_bases_out, last, hipMemcpyDeviceToHost, c->stream));
    if (io.quals_out) HIPCHK(hipMemcpyAsync(io.quals_out, d_quals_out, last, hipMemcpyDeviceToHost, c->stream));
  }
  KCTRY(offs_out.download(c));
  KCTRY(starts.download(c));
  KCTRY(order.download(c));
  KCTRY(home.download(c));
  KCTRY(alns_out.download(c));
  KCTRY(pairs_out.download(c));
  KCTRY(read_back(c, h, a.st));
  if (io.stats) {
    kc_shuffle_stats st;
    memset(&st, 0, sizeof(st));
    st.pairs = npairs;
    st.homed = h[SHS_HOMED];
    st.homeless = npairs - h[SHS_HOMED];
    st.one_mate = h[SHS_ONE_MATE];
    st.two_same = h[SHS_TWO_SAME];
    st.two_diff = h[SHS_TWO_DIFF];
    st.homes = h[SHS_HOMES];
    st.max_home_pairs = h[SHS_MAX_HOME];
    st.bytes = last;
    st.key_bits = (uint64_t)bits;
    *io.stats = st;
  }
  return KC_OK;
}

extern "C" int kc_shuffle_reads(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                                const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs, int on_device, uint32_t parts,
                                uint8_t *bases_out, uint8_t *quals_out, uint64_t *offsets_out, uint32_t *order, uint32_t *home,
                                uint64_t *part_starts, kc_gap_aln *alns_out, kc_pair_rec *pairs_out, kc_shuffle_stats *stats) {
  // the arguments come before the context so that they can be checked where there is no device
  if (nreads & 1)
    return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: %llu reads are no pairs (reads 2p and 2p + 1 are mates)", (unsigned long long)nreads);
  if (parts < 1 || parts > KC_SHUFFLE_MAX_PARTS)
    return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: parts %u outside 1 .. %d", parts, KC_SHUFFLE_MAX_PARTS);
  {
    const void *need[] = {bases_out, offsets_out, order, home, part_starts, nreads ? (const void *)pairs : (const void *)&parts};
    const char *name[] = {"bases_out", "offsets_out", "order", "home", "part_starts", "pairs"};
    for (int i = 0; i < 6; i++)
      if (!need[i]) return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: %s is NULL", name[i]);
  }
  if ((quals == nullptr) != (quals_out == nullptr))
    return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: quals is %s and quals_out is %s: both or neither", quals ? "given" : "NULL",
                quals_out ? "given" : "NULL");
  {
    const void *in[] = {bases, quals, offsets, alns, pairs};
    const char *in_name[] = {"bases", "quals", "offsets", "alns", "pairs"};
    const void *out[] = {bases_out, quals_out, offsets_out, order, home, part_starts, alns_out, pairs_out};
    const char *out_name[] = {"bases_out", "quals_out", "offsets_out", "order", "home", "part_starts", "alns_out", "pairs_out"};
    for (int o = 0; o < 8; o++)
      for (int i = 0; i < 5; i++)
        if (out[o] && out[o] == in[i])
          return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: %s is %s: the call does not work in place", out_name[o], in_name[i]);
  }
  if (!c || (nreads && !offsets) || (n_alns && !alns)) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs | (uintptr_t)alns_out | (uintptr_t)pairs_out) & 15)) return misaligned_records("kc_shuffle_reads");
  if (on_device && ((((uintptr_t)offsets | (uintptr_t)offsets_out | (uintptr_t)part_starts) & 7) || (((uintptr_t)order | (uintptr_t)home) & 3)))
    return fail(KC_ERR_INVALID_ARG, "kc_shuffle_reads: device offsets, offsets_out and part_starts are 8-byte aligned, order and home 4-byte");
  if (!c->ai_ready) return no_ctg_index("kc_shuffle_reads");
  if (nreads > 0xFFFFFFFFull || n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_shuffle_reads: %llu reads and %llu records, an index of either takes 32 bits", (unsigned long long)nreads,
                (unsigned long long)n_alns);
  const ShufIo io{bases,     quals, offsets,     nreads, alns, n_alns,      pairs,    on_device, parts,
                  bases_out, quals_out, offsets_out, order,  home, part_starts, alns_out, pairs_out, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return shuffle_run(c, b, io); });
}
