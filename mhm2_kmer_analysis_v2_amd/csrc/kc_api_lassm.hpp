// kc_api_lassm.hpp -- kc_local_assm (kernels in kc_lassm.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_depth.hpp.

static_assert(sizeof(kc_lassm_params) == 48 && sizeof(kc_lassm_end) == 16 && sizeof(kc_lassm_stats) == 144, "the header's layouts");
static_assert(KC_LASSM_MAX_MER_LEN == LASSM_MAX_MER && KC_LASSM_MAX_WALK == LASSM_MAX_WALK && KC_LASSM_MAX_CANDS == LASSM_MAX_CANDS,
              "the header's limits are the kernels'");
static_assert(KC_LASSM_NO_CANDS == LASSM_NO_CANDS && KC_LASSM_TOO_MANY == LASSM_TOO_MANY && KC_LASSM_DEAD_END == LASSM_DEAD_END &&
                  KC_LASSM_FORK == LASSM_FORK && KC_LASSM_LOOP == LASSM_LOOP && KC_LASSM_MAX_LEN == LASSM_MAX_LEN,
              "the header's statuses");

struct LassmIo {
  const uint8_t *bases, *quals;
  const uint64_t *offsets;
  uint64_t nreads;
  const kc_gap_aln *alns;
  uint64_t n_alns;
  const kc_pair_rec *pairs;
  const kc_ctg_depth *ctgs;
  int on_device;
  uint8_t *seqs_out;
  uint64_t capacity;
  uint64_t *offsets_out;
  kc_lassm_end *ends;
  uint64_t *nbytes_out;
  kc_lassm_stats *stats;
};

static int lassm_run(kc_ctx *c, CallBufs &b, const LassmIo &io, const kc_lassm_params &p) {
  const uint64_t n_ctgs = c->ai.n_ctgs, n_ends = 2 * n_ctgs, nreads = io.nreads, n_alns = io.n_alns, npairs = nreads / 2;
  const bool dev = io.on_device != 0;
  LassmArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  uint64_t *d_als;
  StagedIn<uint64_t> offs = staged_offsets(io.offsets, nreads, dev);
  StagedIn<uint4> alns{io.alns, dev, n_alns * sizeof(kc_gap_aln)}, pairs{io.pairs, dev, npairs * sizeof(kc_pair_rec)};
  StagedIn<uint4> ctgs{io.ctgs, dev, n_ctgs * sizeof(kc_ctg_depth)};
  StagedOut<uint4> ends{io.ends, dev, n_ends * sizeof(kc_lassm_end)};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(LS_COUNT);
    d.st = m.take<uint64_t>(DPS_COUNT);
    d_als = m.take<uint64_t>(ALS_COUNT);
    a.e_cands = m.take<uint64_t>(n_ends);
    a.e_bases = m.take<uint64_t>(n_ends);
    a.e_ecur = m.take<uint32_t>(n_ends);
    a.e_tcur = m.take<uint32_t>(n_ends);
    zeroed = m.used;
    a.e_ent = m.take<uint64_t>(n_ends);
    a.e_text = m.take<uint64_t>(n_ends);
    a.e_slots = m.take<uint64_t>(n_ends);
    a.e_res = m.take<uint4>(n_ends);
    a.newoff = m.take<uint64_t>(n_ctgs + 1);
    a.ext = m.take<uint8_t>(n_ends * p.max_walk_len);
    offs.reserve(m);
    alns.reserve(m);
    pairs.reserve(m);
    ctgs.reserve(m, io.ctgs != nullptr);
    ends.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  KCTRY(alns.upload(c));
  KCTRY(pairs.upload(c));
  KCTRY(ctgs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(a.st + LS_BAD_PAIR, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  const dim3 tpb(256);
  // ---- the checks: nothing is stored through the caller's pointers before the last of them has passed
  uint64_t last;
  KCTRY(check_read_lengths(c, KT_LASSM_LENGTHS, "kc_local_assm", offs.d, nreads, d_als, nullptr, &last));
  if (last && !io.bases) return KC_ERR_INVALID_ARG;
  const uint8_t *d_bases = io.bases, *d_quals = io.quals;
  if (!dev && last) {  // lengths are checked: the reads are the first `last` bytes, the qualities as many behind them
    uint8_t *reads;
    KCTRY(b.alloc(&reads, io.quals ? 2 * last : last));
    HIPCHK(hipMemcpyAsync(reads, io.bases, last, hipMemcpyHostToDevice, c->stream));
    d_bases = reads;
    if (io.quals) {
      HIPCHK(hipMemcpyAsync(reads + last, io.quals, last, hipMemcpyHostToDevice, c->stream));
      d_quals = reads + last;
    }
  }
  KCTRY(check_read_records(c, d, KT_LASSM_CHECK, "kc_local_assm", alns.d, n_alns, offs.d, nreads));
  a.seqs = c->ai.seqs;
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.n_ends = (uint32_t)n_ends;
  a.bases = d_bases;
  a.quals = d_quals;
  a.offsets = offs.d;
  a.nreads = nreads;
  a.alns = alns.d;
  a.n_alns = n_alns;
  a.pairs = pairs.d;
  a.ctgs = ctgs.d;
  a.k = (uint32_t)c->k;
  a.min_mer = p.min_mer_len;
  a.max_mer = p.max_mer_len;
  a.shift = p.shift;
  a.max_walk = p.max_walk_len;
  a.max_insert = p.max_insert;
  a.min_viable = p.min_viable;
  a.permille = p.viable_permille;
  a.max_cands = p.max_cands;
  a.min_q = (int)p.min_qual + c->cfg.qual_offset;
  a.hi_q = (int)p.hi_qual + c->cfg.qual_offset;
  KCTRY(check_pairs(c, a, npairs, KT_LASSM_PAIR_CHECK, "kc_local_assm"));
  // ---- candidates: count, plan, scan
  uint64_t h[LS_COUNT];
  std::vector<uint64_t> slot_off(n_ends + 1, 0);
  if (n_ends) {
    if (nreads) KCTRY(launch_timed(c, KT_LASSM_COUNT, kc_lassm_cands_kernel<false>, blocks_for(nreads), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_PLAN, kc_lassm_plan_kernel, blocks_for(n_ends), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_SCAN, kc_scan_kernel<2>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<2>{{a.e_ent, a.e_text}}, n_ends,
                       a.st + LS_ENT_TOTAL));
    KCTRY(launch_timed(c, KT_LASSM_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.e_slots}}, n_ends, a.st + LS_SLOT_TOTAL));
    HIPCHK(hipMemcpyAsync(slot_off.data(), a.e_slots, n_ends * 8, hipMemcpyDeviceToHost, c->stream));
  }
  KCTRY(read_back(c, h, a.st));
  slot_off[n_ends] = h[LS_SLOT_TOTAL];
  const uint64_t n_ent = h[LS_ENT_TOTAL], n_text = h[LS_TEXT_TOTAL];
  if (n_ent) {
    // ---- batches of ends in index order whose tables fit the budget; an end over the budget runs alone
    const uint64_t budget = ((uint64_t)(p.table_budget_mb ? p.table_budget_mb : 1024) << 20) / (LASSM_SLOT_WORDS * 4);
    std::vector<uint64_t> cuts{0};
    uint64_t most = 0;
    for (uint64_t e = 0; e < n_ends; e++) {
      if (slot_off[e + 1] - slot_off[cuts.back()] > budget && e > cuts.back()) cuts.push_back(e);
      most = std::max(most, slot_off[e + 1] - slot_off[cuts.back()]);
    }
    cuts.push_back(n_ends);
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      a.entries = m.take<uint4>(n_ent);
      a.tph = m.take<uint64_t>(n_text);
      a.tcode = m.take<uint8_t>(n_text);
      a.tnb = m.take<uint8_t>(n_text);
      a.table = m.take<uint32_t>(most * LASSM_SLOT_WORDS);
      return m.used;
    }));
    KCTRY(launch_timed(c, KT_LASSM_SCATTER, kc_lassm_cands_kernel<true>, blocks_for(nreads), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_TEXT, kc_lassm_text_kernel, blocks_for(n_ent), tpb, 0, a, n_ent));
    for (size_t i = 0; i + 1 < cuts.size(); i++) {
      if (slot_off[cuts[i + 1]] == slot_off[cuts[i]]) continue;  // no end of the batch walks
      KCTRY(launch_timed(c, KT_LASSM_WALK, kc_lassm_walk_kernel, dim3((unsigned)(cuts[i + 1] - cuts[i])), dim3(64), 0, a, (uint32_t)cuts[i]));
    }
  }
  // ---- the new block's geometry and the statistics
  if (n_ctgs) {
    KCTRY(launch_timed(c, KT_LASSM_LENS, kc_lassm_lens_kernel, blocks_for(n_ctgs), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.newoff}}, n_ctgs, a.st + LS_OUT_TOTAL));
  }
  HIPCHK(hipMemcpyAsync(a.newoff + n_ctgs, a.st + LS_OUT_TOTAL, 8, hipMemcpyDeviceToDevice, c->stream));
  KCTRY(read_back(c, h, a.st));
  const uint64_t total = h[LS_OUT_TOTAL];
  if (total >= (1ull << 31))
    return fail(KC_ERR_CAPACITY, "kc_local_assm: a block of %llu bytes, a block holds fewer than 2^31", (unsigned long long)total);
  kc_lassm_stats st;
  memset(&st, 0, sizeof(st));
  st.ends = n_ends;
  for (int k = 0; k < LASSM_STATUSES; k++) st.status[k] = h[LS_STATUS + k];
  st.cands_overhang = h[LS_OVERHANG];
  st.cands_mate = h[LS_MATE];
  st.cand_bases = h[LS_CAND_BASES];
  st.iterations = h[LS_ITERS];
  st.ext_bases = h[LS_EXT_BASES];
  st.ctgs_extended = h[LS_EXTENDED];
  if (!io.seqs_out || io.capacity < total) {  // a size query, or too small an array: the totals and nothing else
    *io.nbytes_out = total;
    if (io.stats) *io.stats = st;
    if (!io.seqs_out) return KC_OK;
    return fail(KC_ERR_CAPACITY, "kc_local_assm: a block of %llu bytes, the array holds %llu", (unsigned long long)total,
                (unsigned long long)io.capacity);
  }
  // ---- assemble
  uint8_t *d_out = io.seqs_out;
  if (!dev) KCTRY(b.alloc(&d_out, total));
  if (total) KCTRY(launch_timed(c, KT_LASSM_WRITE, kc_lassm_write_kernel, blocks_for((total + 15) / 16), tpb, 0, a, d_out, total));
  if (io.ends && n_ends) KCTRY(launch_timed(c, KT_LASSM_ENDS, kc_lassm_ends_kernel, blocks_for(n_ends), tpb, 0, a, ends.d));
  const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (io.offsets_out) HIPCHK(hipMemcpyAsync(io.offsets_out, a.newoff, (n_ctgs + 1) * 8, back, c->stream));
  if (!dev && total) HIPCHK(hipMemcpyAsync(io.seqs_out, d_out, total, hipMemcpyDeviceToHost, c->stream));
  KCTRY(ends.download(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  *io.nbytes_out = total;
  if (io.stats) *io.stats = st;
  return KC_OK;
}

extern "C" int kc_local_assm(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                             const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs, const kc_ctg_depth *ctgs, int on_device,
                             const kc_lassm_params *p, uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out, kc_lassm_end *ends,
                             uint64_t *nbytes_out, kc_lassm_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !nbytes_out) return KC_ERR_INVALID_ARG;
  if (p->min_mer_len < 4 || p->min_mer_len > p->max_mer_len || p->max_mer_len > KC_LASSM_MAX_MER_LEN || p->shift < 1 || p->shift > 64)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: mer lengths %u .. %u by %u outside 4 <= min <= max <= %d, 1 <= shift <= 64", p->min_mer_len,
                p->max_mer_len, p->shift, KC_LASSM_MAX_MER_LEN);
  if (p->max_walk_len < 1 || p->max_walk_len > KC_LASSM_MAX_WALK)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: max_walk_len %u outside 1 .. %d", p->max_walk_len, KC_LASSM_MAX_WALK);
  if (p->max_insert < 1 || p->max_insert > KC_INSERT_MAX)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: max_insert %u outside 1 .. %d", p->max_insert, KC_INSERT_MAX);
  if (p->min_qual > p->hi_qual || p->hi_qual > 93)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: qualities %u %u outside min_qual <= hi_qual <= 93", p->min_qual, p->hi_qual);
  if (p->min_viable < 1 || p->viable_permille > 1000)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: min_viable %u under 1 or viable_permille %u over 1000", p->min_viable, p->viable_permille);
  if (p->max_cands < 1 || p->max_cands > KC_LASSM_MAX_CANDS)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: max_cands %u outside 1 .. %u", p->max_cands, KC_LASSM_MAX_CANDS);
  if (p->flags) return fail(KC_ERR_INVALID_ARG, "kc_local_assm: unknown flags 0x%x", p->flags);
  if (nreads & 1)
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: %llu reads are no pairs (reads 2p and 2p + 1 are mates)", (unsigned long long)nreads);
  if (!c || (nreads && (!offsets || !pairs)) || (n_alns && !alns)) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs | (uintptr_t)ctgs | (uintptr_t)ends) & 15)) return misaligned_records("kc_local_assm");
  if (on_device && (((uintptr_t)offsets | (uintptr_t)offsets_out) & 7))
    return fail(KC_ERR_INVALID_ARG, "kc_local_assm: device offsets are 8-byte aligned");
  if (!c->ai_ready) return no_ctg_index("kc_local_assm");
  if (nreads >= (1ull << 30) || n_alns > 0xFFFFFFFFull)
    return fail(KC_ERR_CAPACITY, "kc_local_assm: %llu reads, %llu records: an entry holds a read in 30 bits, a pair an index in 32",
                (unsigned long long)nreads, (unsigned long long)n_alns);
  const LassmIo io{bases, quals, offsets, nreads, alns, n_alns, pairs, ctgs, on_device, seqs_out, capacity, offsets_out, ends, nbytes_out, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return lassm_run(c, b, io, *p); });
}
