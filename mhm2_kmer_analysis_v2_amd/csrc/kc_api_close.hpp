// kc_api_close.hpp -- kc_close_gaps (kernels in kc_close.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_scaffold.hpp; the grouping of the records by read is kc_links.hpp's kernels as kc_api_links.hpp launches them.

static_assert(sizeof(kc_close_params) == 32 && sizeof(kc_closure) == 32 && sizeof(kc_close_stats) == 128, "the header's layouts");
static_assert(KC_CLOSE_HEAD == CLOSE_HEAD && KC_CLOSE_NOT_A_GAP == CLOSE_NOT_A_GAP && KC_CLOSE_NO_READS == CLOSE_NO_READS &&
                  KC_CLOSE_WEAK == CLOSE_WEAK && KC_CLOSE_FILLED == CLOSE_FILLED && KC_CLOSE_ABUT == CLOSE_ABUT &&
                  KC_CLOSE_OVERLAP == CLOSE_OVERLAP && KC_CLOSE_OVERLAP_REJECTED == CLOSE_OVERLAP_REJECTED,
              "the header's statuses");

struct CloseIo {
  const uint8_t *bases;
  const uint64_t *offsets;
  uint64_t nreads;
  const kc_gap_aln *alns;
  uint64_t n_alns;
  const kc_scaffold_rec *scaffolds;
  uint64_t n_scaffolds;
  const kc_scaf_member *members;
  int on_device;
  uint8_t *seqs_out;
  uint64_t capacity;
  uint64_t *offsets_out;
  kc_scaffold_rec *scaffolds_out;
  kc_scaf_member *members_out;
  kc_closure *closures;
  uint64_t *nbytes_out;
  kc_close_stats *stats;
};

static int close_run(kc_ctx *c, CallBufs &b, const CloseIo &io, const kc_close_params &p) {
  const uint32_t n = c->ai.n_ctgs;
  const uint64_t nreads = io.nreads, n_alns = io.n_alns, n_scaf = io.n_scaffolds;
  const uint64_t rtiles = (nreads + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE, mtiles = ((uint64_t)n + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  const bool dev = io.on_device != 0;
  uint64_t nbases = 0;  // the reads' bytes: only a host array's are copied
  if (!dev && nreads) nbases = io.offsets[nreads];
  LinkArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  CloseArgs ca;
  memset(&ca, 0, sizeof(ca));
  uint64_t *st, *d_als, *jcnt, *jbase, *seglen, *segbase, *filllen, *fillbase;
  uint32_t *ishead, *jcur, *owner, *table, *seg, *fill;
  uint4 *dec, *members_w;
  StagedIn<uint64_t> offs = staged_offsets(io.offsets, nreads, dev);
  StagedIn<uint4> alns{io.alns, dev, n_alns * sizeof(kc_gap_aln)}, scaf{io.scaffolds, dev, n_scaf * sizeof(kc_scaffold_rec)};
  StagedIn<uint4> members{io.members, dev, (size_t)n * sizeof(kc_scaf_member)};
  StagedIn<uint8_t> bases{io.bases, dev, nbases};
  size_t zeroed = 0, ff_from = 0, ff_to = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    st = m.take<uint64_t>(CLS_COUNT);
    a.st = m.take<uint64_t>(LKS_COUNT);
    d.st = m.take<uint64_t>(DPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    a.rfirst = m.take<uint64_t>(nreads);
    a.rbase = m.take<uint64_t>(rtiles);
    a.rcur = m.take<uint32_t>(nreads);
    ishead = m.take<uint32_t>(n);
    jcnt = m.take<uint64_t>(n);
    jbase = m.take<uint64_t>(mtiles);
    jcur = m.take<uint32_t>(n);
    zeroed = m.used;
    ff_from = m.used;
    owner = m.take<uint32_t>(n);
    table = m.take<uint32_t>(2 * (uint64_t)n);
    ff_to = m.used;
    seglen = m.take<uint64_t>(n);
    segbase = m.take<uint64_t>(mtiles);
    filllen = m.take<uint64_t>(n);
    fillbase = m.take<uint64_t>(mtiles);
    dec = m.take<uint4>(n);
    seg = m.take<uint32_t>((uint64_t)n + 1);
    fill = m.take<uint32_t>(n);
    members_w = m.take<uint4>(n);
    offs.reserve(m);
    alns.reserve(m);
    scaf.reserve(m);
    members.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(alns.upload(c));
  KCTRY(scaf.upload(c));
  KCTRY(members.upload(c));
  const uint64_t *d_offs = offs.d;
  const uint4 *d_alns = alns.d, *d_scaf = scaf.d, *d_members = members.d;
  HIPCHK(hipMemsetAsync(st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(owner, 0xFF, ff_to - ff_from, c->stream));
  HIPCHK(hipMemsetAsync(st + CLS_BAD, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  auto blocks = [](uint64_t items) { return blocks_for(items, CLOSE_TPB); };
  auto stat_blocks = [](uint64_t items) { return blocks_for(items, LINK_STAT_TPB); };
  const dim3 tpb(CLOSE_TPB), stat_tpb(LINK_STAT_TPB), per_member = blocks(n), per_member_wave = blocks((uint64_t)n * 64);
  // ---- the checks, in the order reads, records, scaffolds, members: nothing is stored before the last has passed
  KCTRY(check_read_lengths(c, KT_CLOSE_LENGTHS, "kc_close_gaps", d_offs, nreads, d_als));
  KCTRY(check_read_records(c, d, KT_CLOSE_CHECK, "kc_close_gaps", d_alns, n_alns, d_offs, nreads));
  KCTRY(launch_timed(c, KT_CLOSE_CHECK_SCAF, kc_close_check_scaf_kernel, blocks(n_scaf), tpb, 0, d_scaf, n_scaf, n, ishead, st));
  KCTRY(lowest_bad(c, st + CLS_BAD,
                   "%s: scaffold %llu is invalid (no member, not where its predecessor ends, or the last does not end at %u members)",
                   "kc_close_gaps", n));
  KCTRY(launch_timed(c, KT_CLOSE_CLAIM, kc_close_claim_kernel, per_member, tpb, 0, (const uint4 *)d_members, n, owner));
  KCTRY(launch_timed(c, KT_CLOSE_CHECK_MEMBER, kc_close_check_member_kernel, per_member, tpb, 0, (const uint4 *)d_members, n,
                     (const uint32_t *)ishead, (const uint32_t *)owner, c->ai.offs, st));
  KCTRY(lowest_bad(c, st + CLS_BAD,
                   "%s: member %llu is invalid (contig or orient out of range, reserved bytes, a contig's second member, a head's join "
                   "not 0, a join out of range or an overlap not shorter than both contigs)",
                   "kc_close_gaps"));
  // ---- the passing records by read, as kc_ctg_links groups them
  a.offs = c->ai.offs;
  a.n_ctgs = n;
  a.alns = d_alns;
  a.n_alns = n_alns;
  a.offsets = d_offs;
  a.nreads = nreads;
  a.min_score = p.min_score;
  a.min_len = p.min_len;
  a.end_slack = p.end_slack;
  a.max_overlap = p.max_overlap;
  a.max_splint_gap = p.max_splint_gap;
  a.max_read_alns = p.max_read_alns;
  uint64_t slots = 0, n_cands = 0;
  if (n_alns && nreads) {
    KCTRY(launch_timed(c, KT_CLOSE_GROUP_COUNT, kc_link_group_kernel<false>, stat_blocks(n_alns), stat_tpb, 0, a));
    KCTRY(tiled_scan(c, KT_CLOSE_TILE_SCAN, KT_CLOSE_SCAN, a.rfirst, nreads, a.rbase, a.st + LKS_SLOT_TOTAL));
    KCTRY(read_back(c, &slots, a.st + LKS_SLOT_TOTAL, 1));
  }
  // ---- the gap joins' ends, and the candidates: count, scan, write
  KCTRY(launch_timed(c, KT_CLOSE_ENDS, kc_close_ends_kernel, per_member, tpb, 0, (const uint4 *)d_members, n, (const uint32_t *)ishead, table));
  ca.offsets = d_offs;
  ca.nreads = nreads;
  ca.rfirst = a.rfirst;
  ca.rbase = a.rbase;
  ca.rcur = a.rcur;
  ca.table = table;
  ca.max_overlap = p.max_overlap;
  ca.max_splint_gap = p.max_splint_gap;
  ca.max_read_alns = p.max_read_alns;
  ca.jcnt = jcnt;
  ca.jbase = jbase;
  ca.jcur = jcur;
  ca.st = st;
  if (slots) {
    // the slots, and a host array's read bytes: behind the checks, so that no bad offset sizes an allocation
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      a.info = m.take<uint4>(slots);
      bases.reserve(m);
      return m.used;
    }));
    KCTRY(bases.upload(c));
    ca.info = a.info;
    KCTRY(launch_timed(c, KT_CLOSE_GROUP_FILL, kc_link_group_kernel<true>, blocks(n_alns), tpb, 0, a));
    KCTRY(launch_timed(c, KT_CLOSE_CANDS_COUNT, kc_close_cands_kernel<false>, stat_blocks(nreads), stat_tpb, 0, ca));
    KCTRY(tiled_scan(c, KT_CLOSE_TILE_SCAN, KT_CLOSE_SCAN, jcnt, n, jbase, st + CLS_JCAND_TOTAL));
    KCTRY(read_back(c, &n_cands, st + CLS_JCAND_TOTAL, 1));
    if (n_cands) {
      KCTRY(b.alloc(&ca.cands, n_cands * sizeof(uint4)));
      KCTRY(launch_timed(c, KT_CLOSE_CANDS_WRITE, kc_close_cands_kernel<true>, blocks(nreads), tpb, 0, ca));
    }
  }
  // ---- a decision a member, and where its bytes go
  KCTRY(launch_timed(c, KT_CLOSE_DECIDE, kc_close_decide_kernel, per_member_wave, tpb, 0, (const uint4 *)d_members, n, (const uint32_t *)ishead,
                     (const uint64_t *)jcnt, (const uint64_t *)jbase, (const uint32_t *)jcur, (const uint4 *)ca.cands, p.min_reads,
                     p.min_agree_permille, c->ai.seqs, c->ai.offs, dec, seglen, filllen));
  KCTRY(tiled_scan(c, KT_CLOSE_TILE_SCAN, KT_CLOSE_SCAN, seglen, n, segbase, st + CLS_SEG_TOTAL));
  KCTRY(tiled_scan(c, KT_CLOSE_TILE_SCAN, KT_CLOSE_SCAN, filllen, n, fillbase, st + CLS_FILL_TOTAL));
  uint64_t h[CLS_COUNT], hl[LKS_COUNT];
  HIPCHK(hipMemcpyAsync(h, st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  KCTRY(read_back(c, hl, a.st));
  const uint64_t total = h[CLS_SEG_TOTAL], fill_total = h[CLS_FILL_TOTAL];
  if (total >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_close_gaps: the scaffolds are %llu bytes, a block holds fewer than 2^31", (unsigned long long)total);
  const bool fits = io.seqs_out && io.capacity >= total;
  const bool want_recs = fits && io.scaffolds_out != nullptr;
  uint8_t *buf = nullptr;
  uint32_t *acc = nullptr;
  StagedOut<uint8_t> seqs{io.seqs_out, dev, total};
  StagedOut<uint64_t> offsets{io.offsets_out, dev, (n_scaf + 1) * 8};
  StagedOut<uint4> scaf_out{io.scaffolds_out, dev, n_scaf * sizeof(kc_scaffold_rec)}, members_out{io.members_out, dev, (size_t)n * sizeof(kc_scaf_member)};
  StagedOut<uint4> closures{io.closures, dev, (size_t)n * sizeof(kc_closure)};
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    buf = m.take<uint8_t>(fill_total);
    acc = m.take<uint32_t>(2 * n_scaf);
    seqs.reserve(m, fits);
    offsets.reserve(m, fits);
    scaf_out.reserve(m, fits);
    members_out.reserve(m, fits);
    closures.reserve(m, fits);
    return m.used;
  }));
  uint8_t *const d_seqs = seqs.d;
  uint64_t *const d_offsets = offsets.d;
  uint4 *const d_scaf_out = scaf_out.d, *const d_members_out = members_out.d, *const d_closures = closures.d;
  HIPCHK(hipMemsetAsync(acc, 0, 2 * n_scaf * 4, c->stream));
  KCTRY(launch_timed(c, KT_CLOSE_PLACE, kc_close_place_kernel, stat_blocks(n), stat_tpb, 0, (const uint4 *)d_members, n, (const uint4 *)dec,
                     (const uint64_t *)seglen, (const uint64_t *)segbase, (const uint64_t *)filllen, (const uint64_t *)fillbase, (uint32_t)total,
                     (const uint4 *)d_scaf, n_scaf, seg, fill, members_w, d_members_out, d_closures, want_recs ? acc : (uint32_t *)nullptr, st));
  if (fill_total)
    KCTRY(launch_timed(c, KT_CLOSE_VOTE, kc_close_vote_kernel, stat_blocks((uint64_t)n * 64), stat_tpb, 0, (const uint4 *)dec, n, (const uint64_t *)jcnt,
                       (const uint64_t *)jbase, (const uint32_t *)jcur, (const uint4 *)ca.cands, (const uint8_t *)bases.d,
                       (const uint32_t *)fill, buf, d_closures, st));
  if (fits) {
    if (d_offsets || d_scaf_out)
      KCTRY(launch_timed(c, KT_CLOSE_RECORDS, kc_close_records_kernel, blocks(n_scaf), tpb, 0, (const uint4 *)d_scaf, n_scaf, (const uint32_t *)seg,
                         (const uint32_t *)acc, (uint32_t)total, d_scaf_out, d_offsets));
    const uint32_t mis = (uint32_t)((uintptr_t)d_seqs & 15);
    KCTRY(launch_timed(c, KT_CLOSE_WRITE, kc_close_write_kernel, blocks((total + mis + 15) / 16), tpb, 0, (const uint4 *)members_w,
                       (const uint32_t *)seg, (const uint32_t *)fill, n, c->ai.seqs, c->ai.offs, (const uint8_t *)buf, mis, (uint32_t)total,
                       d_seqs));
    KCTRY(seqs.download(c));
    KCTRY(offsets.download(c));
    KCTRY(scaf_out.download(c));
    KCTRY(members_out.download(c));
    KCTRY(closures.download(c));
  }
  KCTRY(read_back(c, h, st));  // again: the place kernel and the vote count
  *io.nbytes_out = total;
  if (io.stats) {
    kc_close_stats s;
    memset(&s, 0, sizeof(s));
    s.members = n;
    s.joins = n - n_scaf;
    s.gaps = h[CLS_GAPS];
    s.reads_over_cap = h[CLS_OVER_CAP];
    s.passed = hl[LKS_PASSED];
    s.cands = h[CLS_CANDS];
    s.cands_off_join = h[CLS_OFF_JOIN];
    s.gaps_no_reads = h[CLS_NO_READS];
    s.gaps_weak = h[CLS_WEAK];
    s.filled = h[CLS_FILLED];
    s.abutted = h[CLS_ABUT];
    s.overlapped = h[CLS_OVERLAP];
    s.overlaps_rejected = h[CLS_OV_REJECTED];
    s.fill_bases = h[CLS_FILL_BASES];
    s.n_bases_left = h[CLS_N_LEFT];
    s.disputed_cols = h[CLS_DISPUTED];
    *io.stats = s;
  }
  if (io.seqs_out && !fits)
    return fail(KC_ERR_CAPACITY, "kc_close_gaps: %llu bytes, the array holds %llu", (unsigned long long)total, (unsigned long long)io.capacity);
  return KC_OK;
}

extern "C" int kc_close_gaps(kc_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns,
                             const kc_scaffold_rec *scaffolds, uint64_t n_scaffolds, const kc_scaf_member *members, int on_device,
                             const kc_close_params *p, uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out,
                             kc_scaffold_rec *scaffolds_out, kc_scaf_member *members_out, kc_closure *closures, uint64_t *nbytes_out,
                             kc_close_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !nbytes_out) return KC_ERR_INVALID_ARG;
  if (p->end_slack > KC_LINK_MAX_SLACK) return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: end_slack %u over %d", p->end_slack, KC_LINK_MAX_SLACK);
  if (p->max_overlap > KC_LINK_MAX_OVERLAP || p->max_splint_gap > KC_LINK_MAX_SLACK)
    return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: max_overlap %u over %d or max_splint_gap %u over %d", p->max_overlap, KC_LINK_MAX_OVERLAP,
                p->max_splint_gap, KC_LINK_MAX_SLACK);
  if (p->min_reads < 1) return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: min_reads %u below 1", p->min_reads);
  if (p->min_agree_permille > 1000) return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: min_agree_permille %u over 1000", p->min_agree_permille);
  if (p->max_read_alns < 2 || p->max_read_alns > KC_LINK_MAX_READ_ALNS)
    return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: max_read_alns %u outside 2 .. %d", (unsigned)p->max_read_alns, KC_LINK_MAX_READ_ALNS);
  if (p->flags) return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: unknown flags 0x%x", (unsigned)p->flags);
  if (!c || (nreads && (!offsets || !bases)) || (n_alns && !alns) || !scaffolds || !members || nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)scaffolds | (uintptr_t)members | (uintptr_t)scaffolds_out | (uintptr_t)members_out |
                     (uintptr_t)closures) & 15))
    return misaligned_records("kc_close_gaps");
  if (on_device && (((uintptr_t)offsets | (uintptr_t)offsets_out) & 7))
    return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: device offsets are 8-byte aligned");
  if (!c->ai_ready) return no_ctg_index("kc_close_gaps");
  if (c->ai.n_ctgs == 0 || c->ai.n_ctgs >= (1u << 31))
    return fail(c->ai.n_ctgs ? KC_ERR_CAPACITY : KC_ERR_STATE, "kc_close_gaps: %u contigs, oriented node ids are 32-bit (1 .. 2^31 - 1 contigs)",
                c->ai.n_ctgs);
  if (n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_close_gaps: %llu records, a join counts its candidates in 32 bits", (unsigned long long)n_alns);
  if (n_scaffolds == 0) return fail(KC_ERR_INVALID_ARG, "kc_close_gaps: scaffold 0 is invalid (no scaffolds over %u contigs)", c->ai.n_ctgs);
  const CloseIo io{bases,    offsets,     nreads,        alns,        n_alns,   scaffolds,  n_scaffolds, members, on_device,
                   seqs_out, capacity,    offsets_out,   scaffolds_out, members_out, closures, nbytes_out,  stats};
  return call_with_bufs(c, [&](CallBufs &b) { return close_run(c, b, io, *p); });
}
