// kc_api_scaffold.hpp -- kc_scaffold (kernels in kc_scaffold.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_links.hpp; the jump rounds' count is kc_api_unitig.hpp's.

static_assert(sizeof(kc_scaf_params) == 32 && sizeof(kc_scaffold_rec) == 32 && sizeof(kc_scaf_member) == 16 && sizeof(kc_scaf_stats) == 160,
              "the header's layouts");
static_assert(KC_SCAF_MAX_SLACK == SCAF_MAX_SLACK && KC_SCAF_CIRCULAR == SCAF_CIRCULAR, "the header's limits are the kernels'");

struct ScafIo {
  const kc_ctg_link *links;
  uint64_t n_links;
  int on_device;
  uint8_t *seqs_out;
  uint64_t capacity;
  uint64_t *offsets_out;
  kc_scaffold_rec *scaffolds;
  kc_scaf_member *members;
  uint32_t *ctg_member;
  uint64_t *n_scaffolds, *nbytes_out;
  kc_scaf_stats *stats;
};

static int scaffold_run(kc_ctx *c, CallBufs &b, const ScafIo &io, const kc_scaf_params &p) {
  const uint32_t n = c->ai.n_ctgs, nn = 2 * n;
  const uint64_t n_ends = nn, n_links = io.n_links;
  const bool dev = io.on_device != 0;
  uint64_t *st, *keys, *end_first, *size, *num, *mcnt;
  uint4 *pick, *info;
  uint2 *link, *next2, *cyc[2], *rank[2], *pos[2];
  StagedIn<uint4> links{io.links, dev, n_links * sizeof(kc_ctg_link)};
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    st = m.take<uint64_t>(SCS_COUNT);
    size = m.take<uint64_t>(n);
    num = m.take<uint64_t>(n);
    mcnt = m.take<uint64_t>(n);
    info = m.take<uint4>(n);
    keys = m.take<uint64_t>(n_links);
    end_first = m.take<uint64_t>(n_ends + 1);
    pick = m.take<uint4>(n_ends);
    link = m.take<uint2>(n_ends);
    next2 = m.take<uint2>(n);
    for (auto &q : cyc) q = m.take<uint2>(nn);
    for (auto &q : rank) q = m.take<uint2>(nn);
    for (auto &q : pos) q = m.take<uint2>(nn);
    links.reserve(m);
    return m.used;
  }));
  const uint4 *d_links = links.d;
  // st .. info are neighbours in the layout
  HIPCHK(hipMemsetAsync(st, 0, (size_t)((uint8_t *)keys - (uint8_t *)st), c->stream));
  HIPCHK(hipMemsetAsync(st + SCS_BAD, 0xFF, 8, c->stream));
  KCTRY(links.upload(c));
  auto blocks = [](uint64_t items) { return blocks_for(items, SCAF_TPB); };
  const dim3 tpb(SCAF_TPB), per_ctg = blocks(n), per_node = blocks(nn), per_end_wave = blocks(n_ends * 64);
  // ---- the check: its verdict is read before anything is stored
  if (n_links) {
    KCTRY(launch_timed(c, KT_SCAF_CHECK, kc_scaf_check_kernel, blocks(n_links), tpb, 0, d_links, n_links, n_ends, keys, st));
    KCTRY(lowest_bad(c, st + SCS_BAD,
                     "%s: record %llu is invalid (an end out of range, two ends of one contig, no supporter, figures out of range, "
                     "not above its predecessor, or no mirror with the same figures)",
                     "kc_scaffold"));
  }
  // ---- one partner an end, the overlaps, next[]
  KCTRY(launch_timed(c, KT_SCAF_END_FIRST, kc_link_end_first_kernel, blocks(n_ends + 1), tpb, 0, (const uint64_t *)keys, n_links, n_ends, end_first));
  KCTRY(launch_timed(c, KT_SCAF_CHOOSE, kc_scaf_choose_kernel, per_end_wave, tpb, 0, d_links, (const uint64_t *)end_first, n_ends,
                     p.min_splints, p.min_spans, p.max_second_permille, pick, st));
  KCTRY(launch_timed(c, KT_SCAF_EDGE, kc_scaf_edge_kernel, per_end_wave, tpb, 0, (const uint4 *)pick, n_ends, c->ai.seqs, c->ai.offs, p.overlap_slack,
                     link, st));
  KCTRY(launch_timed(c, KT_SCAF_NEXT, kc_scaf_next_kernel, per_ctg, tpb, 0, (const uint2 *)link, n, next2, (uint4 *)cyc[0]));
  // ---- cycles, the cut, and the two rankings: members before a node, and where its text starts
  const int rounds = unitig_rounds(n);
  int cur = 0;
  for (int r = 0; r < rounds; r++, cur ^= 1)
    KCTRY(launch_timed(c, KT_SCAF_MIN_JUMP, kc_unitig_min_jump_kernel, per_node, tpb, 0, (const uint2 *)cyc[cur], cyc[cur ^ 1], nn));
  KCTRY(launch_timed(c, KT_SCAF_CUT, kc_unitig_cut_kernel, per_ctg, tpb, 0, (const uint4 *)cyc[cur], next2, (uint4 *)rank[0], n, st));
  KCTRY(launch_timed(c, KT_SCAF_WEIGHT, kc_scaf_weight_kernel, per_ctg, tpb, 0, (const uint4 *)rank[0], (const uint2 *)next2, (const uint2 *)link,
                     c->ai.offs, n, (uint4 *)pos[0], st));
  uint64_t h[SCS_COUNT];
  KCTRY(read_back(c, h, st));
  // every path is counted with its twin: half the tails are scaffolds, half the bytes theirs
  const uint64_t total = h[SCS_BYTES2] / 2 + h[SCS_TAILS] / 2;
  if (total >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_scaffold: the scaffolds are %llu bytes, a block holds fewer than 2^31", (unsigned long long)total);
  int rk = 0;
  for (int r = 0; r < rounds; r++, rk ^= 1) {
    KCTRY(launch_timed(c, KT_SCAF_RANK_JUMP, kc_unitig_rank_jump_kernel, per_node, tpb, 0, (const uint2 *)rank[rk], rank[rk ^ 1], nn));
    KCTRY(launch_timed(c, KT_SCAF_POS_JUMP, kc_unitig_rank_jump_kernel, per_node, tpb, 0, (const uint2 *)pos[rk], pos[rk ^ 1], nn));
  }
  KCTRY(launch_timed(c, KT_SCAF_SELECT, kc_scaf_select_kernel, per_node, tpb, 0, (const uint2 *)rank[rk], (const uint2 *)pos[rk], (const uint2 *)cyc[cur],
                     (const uint32_t *)next2, c->ai.offs, nn, size, num, mcnt, info, st));
  KCTRY(launch_timed(c, KT_SCAF_SCAN, kc_scan_kernel<2>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<2>{{size, num}}, (uint64_t)n, st + SCS_TOTALS));
  KCTRY(launch_timed(c, KT_SCAF_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{mcnt}}, (uint64_t)n, st + SCS_MTOTAL));
  KCTRY(read_back(c, h, st));
  const uint64_t n_scaf = h[SCS_TOTALS + 1];
  if (h[SCS_TOTALS] != total || h[SCS_MTOTAL] != n)
    return fail(KC_ERR_STATE, "kc_scaffold: the walk gives %llu bytes and %llu members, the sums %llu and %u", (unsigned long long)h[SCS_TOTALS],
                (unsigned long long)h[SCS_MTOTAL], (unsigned long long)total, n);
  kc_scaf_stats s;
  memset(&s, 0, sizeof(s));
  s.contigs = n;
  s.records = n_links;
  s.qualifying = h[SCS_QUALIFYING];
  s.ends_best = h[SCS_ENDS_BEST];
  s.ends_ambiguous = h[SCS_AMBIGUOUS];
  s.ends_not_mutual = h[SCS_NOT_MUTUAL];
  s.edges_chosen = h[SCS_CHOSEN];
  s.overlaps_checked = h[SCS_OV_CHECKED];
  s.overlaps_rejected = h[SCS_OV_REJECTED];
  s.edges_joined = h[SCS_JOINED];
  s.scaffolds = n_scaf;
  s.singletons = h[SCS_SINGLE];
  s.circular = h[SCS_CIRCULAR];
  s.bases = total - n_scaf;
  s.n_bases = h[SCS_N2] / 2;
  s.overlap_bases = h[SCS_OV2] / 2;
  s.longest = h[SCS_LONGEST];
  const bool fits = io.seqs_out && io.capacity >= total;
  if (fits) {
    uint32_t *seg, *acc;
    StagedOut<uint8_t> seqs{io.seqs_out, dev, total};
    StagedOut<uint64_t> offsets{io.offsets_out, dev, (n_scaf + 1) * 8};
    StagedOut<uint4> scaf{io.scaffolds, dev, n_scaf * sizeof(kc_scaffold_rec)}, members{io.members, dev, (size_t)n * sizeof(kc_scaf_member)};
    StagedOut<uint32_t> cm{io.ctg_member, dev, (size_t)n * 4};
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      seg = m.take<uint32_t>((uint64_t)n + 1);
      acc = m.take<uint32_t>(2 * n_scaf);
      members.reserve(m);
      if (!io.members) members.d = m.take<uint4>(n);  // the write kernel reads them, whoever else wants them
      seqs.reserve(m);
      offsets.reserve(m);
      scaf.reserve(m);
      cm.reserve(m);
      return m.used;
    }));
    uint8_t *const d_seqs = seqs.d;
    HIPCHK(hipMemsetAsync(acc, 0, 2 * n_scaf * 4, c->stream));
    KCTRY(launch_timed(c, KT_SCAF_MEMBERS, kc_scaf_members_kernel, per_node, tpb, 0, (const uint2 *)rank[rk], (const uint2 *)pos[rk], (const uint2 *)link,
                       (const uint4 *)info, (const uint64_t *)size, (const uint64_t *)num, (const uint64_t *)mcnt, nn, (uint32_t)total, n_scaf,
                       members.d, seg, acc, offsets.d, cm.d));
    if (scaf.d)
      KCTRY(launch_timed(c, KT_SCAF_RECORDS, kc_scaf_records_kernel, per_ctg, tpb, 0, (const uint4 *)info, (const uint64_t *)num,
                         (const uint64_t *)mcnt, (const uint32_t *)acc, n, scaf.d));
    const uint32_t mis = (uint32_t)((uintptr_t)d_seqs & 15);
    KCTRY(launch_timed(c, KT_SCAF_WRITE, kc_scaf_write_kernel, blocks((total + mis + 15) / 16), tpb, 0, (const uint4 *)members.d,
                       (const uint32_t *)seg, n, c->ai.seqs, c->ai.offs, mis, (uint32_t)total, d_seqs));
    KCTRY(seqs.download(c));
    KCTRY(offsets.download(c));
    KCTRY(scaf.download(c));
    KCTRY(members.download(c));
    KCTRY(cm.download(c));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  *io.n_scaffolds = n_scaf;
  *io.nbytes_out = total;
  if (io.stats) *io.stats = s;
  if (io.seqs_out && !fits)
    return fail(KC_ERR_CAPACITY, "kc_scaffold: %llu bytes, the array holds %llu", (unsigned long long)total, (unsigned long long)io.capacity);
  return KC_OK;
}

extern "C" int kc_scaffold(kc_ctx *c, const kc_ctg_link *links, uint64_t n_links, int on_device, const kc_scaf_params *p, uint8_t *seqs_out,
                           uint64_t capacity, uint64_t *offsets_out, kc_scaffold_rec *scaffolds, kc_scaf_member *members, uint32_t *ctg_member,
                           uint64_t *n_scaffolds, uint64_t *nbytes_out, kc_scaf_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_scaffolds || !nbytes_out) return KC_ERR_INVALID_ARG;
  if (p->min_splints < 1 || p->min_spans < 1)
    return fail(KC_ERR_INVALID_ARG, "kc_scaffold: min_splints %u, min_spans %u below 1", p->min_splints, p->min_spans);
  if (p->max_second_permille > 1000) return fail(KC_ERR_INVALID_ARG, "kc_scaffold: max_second_permille %u over 1000", p->max_second_permille);
  if (p->overlap_slack > KC_SCAF_MAX_SLACK)
    return fail(KC_ERR_INVALID_ARG, "kc_scaffold: overlap_slack %u over %d", p->overlap_slack, KC_SCAF_MAX_SLACK);
  if (p->flags || p->reserved[0] || p->reserved[1] || p->reserved[2])
    return fail(KC_ERR_INVALID_ARG, "kc_scaffold: unknown flags 0x%x", (unsigned)(p->flags | p->reserved[0] | p->reserved[1] | p->reserved[2]));
  if (!c || (n_links && !links)) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)links | (uintptr_t)scaffolds | (uintptr_t)members) & 15)) return misaligned_records("kc_scaffold");
  if (on_device && ((((uintptr_t)offsets_out) & 7) || (((uintptr_t)ctg_member) & 3)))
    return fail(KC_ERR_INVALID_ARG, "kc_scaffold: device offsets are 8-byte aligned, ctg_member 4-byte");
  if (!c->ai_ready) return no_ctg_index("kc_scaffold");
  if (c->ai.n_ctgs == 0 || c->ai.n_ctgs >= (1u << 31))
    return fail(c->ai.n_ctgs ? KC_ERR_CAPACITY : KC_ERR_STATE, "kc_scaffold: %u contigs, oriented node ids are 32-bit (1 .. 2^31 - 1 contigs)",
                c->ai.n_ctgs);
  const ScafIo io{links, n_links, on_device, seqs_out, capacity, offsets_out, scaffolds, members, ctg_member, n_scaffolds, nbytes_out, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return scaffold_run(c, b, io, *p); });
}
