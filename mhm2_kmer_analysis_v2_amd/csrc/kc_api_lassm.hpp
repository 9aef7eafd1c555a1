// kc_api_lassm.hpp -- kc_local_assm (kernels in kc_lassm.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_depth.hpp, whose record check it launches; the length check is kc_api_align.hpp's.

static_assert(sizeof(kc_lassm_params) == 48 && sizeof(kc_lassm_end) == 16 && sizeof(kc_lassm_stats) == 144, "the header's layouts");
static_assert(KC_LASSM_MAX_MER_LEN == LASSM_MAX_MER && KC_LASSM_MAX_WALK == LASSM_MAX_WALK && KC_LASSM_MAX_CANDS == LASSM_MAX_CANDS,
              "the header's limits are the kernels'");
static_assert(KC_LASSM_NO_CANDS == LASSM_NO_CANDS && KC_LASSM_TOO_MANY == LASSM_TOO_MANY && KC_LASSM_DEAD_END == LASSM_DEAD_END &&
                  KC_LASSM_FORK == LASSM_FORK && KC_LASSM_LOOP == LASSM_LOOP && KC_LASSM_MAX_LEN == LASSM_MAX_LEN,
              "the header's statuses");

// device memory the call holds until it returns
struct LassmBufs {
  uint8_t *p[4] = {nullptr, nullptr, nullptr, nullptr};
  void release() {
    for (auto &q : p) {
      if (q) (void)hipFree(q);
      q = nullptr;
    }
  }
};

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

static int lassm_run(kc_ctx *c, LassmBufs &b, const LassmIo &io, const kc_lassm_params &p) {
  const uint64_t n_ctgs = c->ai.n_ctgs, n_ends = 2 * n_ctgs, nreads = io.nreads, n_alns = io.n_alns, npairs = nreads / 2;
  const bool dev = io.on_device != 0;
  LassmArgs a;
  memset(&a, 0, sizeof(a));
  DepthArgs d;
  memset(&d, 0, sizeof(d));
  uint64_t *d_als, *d_offs = nullptr;
  uint4 *d_alns = nullptr, *d_pairs = nullptr, *d_ctgs = nullptr, *d_ends = nullptr;
  size_t zeroed = 0;
  auto layout = [&](uint8_t *base) {
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
    if (!dev) {
      d_offs = m.take<uint64_t>(nreads + 1);
      d_alns = m.take<uint4>(2 * n_alns);
      d_pairs = m.take<uint4>(npairs);
      if (io.ctgs) d_ctgs = m.take<uint4>(2 * n_ctgs);
      if (io.ends) d_ends = m.take<uint4>(n_ends);
    }
    return m.used;
  };
  HIPCHK(hipMalloc((void **)&b.p[0], layout(nullptr)));
  layout(b.p[0]);
  if (dev) {
    d_offs = const_cast<uint64_t *>(io.offsets);
    d_alns = (uint4 *)const_cast<kc_gap_aln *>(io.alns);
    d_pairs = (uint4 *)const_cast<kc_pair_rec *>(io.pairs);
    d_ctgs = (uint4 *)const_cast<kc_ctg_depth *>(io.ctgs);
    d_ends = (uint4 *)io.ends;
  } else {
    if (nreads) HIPCHK(hipMemcpyAsync(d_offs, io.offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_alns) HIPCHK(hipMemcpyAsync(d_alns, io.alns, n_alns * sizeof(kc_gap_aln), hipMemcpyHostToDevice, c->stream));
    if (npairs) HIPCHK(hipMemcpyAsync(d_pairs, io.pairs, npairs * sizeof(kc_pair_rec), hipMemcpyHostToDevice, c->stream));
    if (io.ctgs && n_ctgs) HIPCHK(hipMemcpyAsync(d_ctgs, io.ctgs, n_ctgs * sizeof(kc_ctg_depth), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  HIPCHK(hipMemsetAsync(a.st + LS_BAD_PAIR, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d.st + DPS_BAD, 0xFF, 8, c->stream));
  HIPCHK(hipMemsetAsync(d_als + ALS_BAD_READ, 0xFF, 8, c->stream));
  auto blocks = [](uint64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  const dim3 tpb(256);
  // ---- the checks: nothing is stored through the caller's pointers before the last of them has passed
  uint64_t last = 0;
  if (nreads) {
    KCTRY(launch_timed(c, KT_LASSM_LENGTHS, kc_align_lengths_kernel, blocks(nreads), tpb, 0, (const uint64_t *)d_offs, nreads, d_als));
    uint64_t bad_read = ~0ull;
    HIPCHK(hipMemcpyAsync(&bad_read, d_als + ALS_BAD_READ, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&last, d_offs + nreads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad_read != ~0ull) {
      snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: read %llu is longer than %d bases, or its offsets decrease",
               (unsigned long long)bad_read, KC_ALIGN_MAX_READ_LEN);
      return KC_ERR_INVALID_ARG;
    }
  }
  if (last && !io.bases) return KC_ERR_INVALID_ARG;
  const uint8_t *d_bases = io.bases, *d_quals = io.quals;
  if (!dev && last) {  // lengths are checked: the reads are the first `last` bytes
    HIPCHK(hipMalloc((void **)&b.p[1], io.quals ? 2 * last : last));
    HIPCHK(hipMemcpyAsync(b.p[1], io.bases, last, hipMemcpyHostToDevice, c->stream));
    d_bases = b.p[1];
    if (io.quals) {
      HIPCHK(hipMemcpyAsync(b.p[1] + last, io.quals, last, hipMemcpyHostToDevice, c->stream));
      d_quals = b.p[1] + last;
    }
  }
  d.offs = c->ai.offs;
  d.n_ctgs = (uint32_t)n_ctgs;
  d.nbytes = (uint32_t)c->ai_nbytes;
  d.alns = d_alns;
  d.n_alns = n_alns;
  d.nreads = nreads;
  d.offsets = d_offs;
  KCTRY(depth_check(c, d, KT_LASSM_CHECK, 1, "kc_local_assm"));
  a.seqs = c->ai.seqs;
  a.offs = c->ai.offs;
  a.n_ctgs = (uint32_t)n_ctgs;
  a.n_ends = (uint32_t)n_ends;
  a.bases = d_bases;
  a.quals = d_quals;
  a.offsets = d_offs;
  a.nreads = nreads;
  a.alns = d_alns;
  a.n_alns = n_alns;
  a.pairs = d_pairs;
  a.ctgs = d_ctgs;
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
  if (npairs) {
    KCTRY(launch_timed(c, KT_LASSM_PAIR_CHECK, kc_lassm_pair_check_kernel, blocks(npairs), tpb, 0, a));
    uint64_t bad = ~0ull;
    HIPCHK(hipMemcpyAsync(&bad, a.st + LS_BAD_PAIR, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad != ~0ull) {
      snprintf(g_last_error, sizeof(g_last_error),
               "kc_local_assm: pair %llu names a record that is out of range, of another read or of kind KC_GAP_NONE", (unsigned long long)bad);
      return KC_ERR_INVALID_ARG;
    }
  }
  // ---- candidates: count, plan, scan
  uint64_t h[LS_COUNT];
  std::vector<uint64_t> slot_off(n_ends + 1, 0);
  if (n_ends) {
    if (nreads) KCTRY(launch_timed(c, KT_LASSM_COUNT, kc_lassm_cands_kernel<false>, blocks(nreads), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_PLAN, kc_lassm_plan_kernel, blocks(n_ends), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_SCAN, kc_scan_kernel<2>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<2>{{a.e_ent, a.e_text}}, n_ends,
                       a.st + LS_ENT_TOTAL));
    KCTRY(launch_timed(c, KT_LASSM_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.e_slots}}, n_ends, a.st + LS_SLOT_TOTAL));
    HIPCHK(hipMemcpyAsync(slot_off.data(), a.e_slots, n_ends * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(h, a.st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
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
    auto work = [&](uint8_t *base) {
      Carver m{base, 0};
      a.entries = m.take<uint4>(n_ent);
      a.tph = m.take<uint64_t>(n_text);
      a.tcode = m.take<uint8_t>(n_text);
      a.tnb = m.take<uint8_t>(n_text);
      a.table = m.take<uint32_t>(most * LASSM_SLOT_WORDS);
      return m.used;
    };
    HIPCHK(hipMalloc((void **)&b.p[2], work(nullptr)));
    work(b.p[2]);
    KCTRY(launch_timed(c, KT_LASSM_SCATTER, kc_lassm_cands_kernel<true>, blocks(nreads), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_TEXT, kc_lassm_text_kernel, blocks(n_ent), tpb, 0, a, n_ent));
    for (size_t i = 0; i + 1 < cuts.size(); i++) {
      if (slot_off[cuts[i + 1]] == slot_off[cuts[i]]) continue;  // no end of the batch walks
      KCTRY(launch_timed(c, KT_LASSM_WALK, kc_lassm_walk_kernel, dim3((unsigned)(cuts[i + 1] - cuts[i])), dim3(64), 0, a, (uint32_t)cuts[i]));
    }
  }
  // ---- the new block's geometry and the statistics
  if (n_ctgs) {
    KCTRY(launch_timed(c, KT_LASSM_LENS, kc_lassm_lens_kernel, blocks(n_ctgs), tpb, 0, a));
    KCTRY(launch_timed(c, KT_LASSM_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.newoff}}, n_ctgs, a.st + LS_OUT_TOTAL));
  }
  HIPCHK(hipMemcpyAsync(a.newoff + n_ctgs, a.st + LS_OUT_TOTAL, 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(h, a.st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t total = h[LS_OUT_TOTAL];
  if (total >= (1ull << 31)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: a block of %llu bytes, a block holds fewer than 2^31", (unsigned long long)total);
    return KC_ERR_CAPACITY;
  }
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
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: a block of %llu bytes, the array holds %llu", (unsigned long long)total,
             (unsigned long long)io.capacity);
    return KC_ERR_CAPACITY;
  }
  // ---- assemble
  uint8_t *d_out = io.seqs_out;
  if (!dev && total) {
    HIPCHK(hipMalloc((void **)&b.p[3], total));
    d_out = b.p[3];
  }
  if (total) KCTRY(launch_timed(c, KT_LASSM_WRITE, kc_lassm_write_kernel, blocks((total + 15) / 16), tpb, 0, a, d_out, total));
  if (io.ends && n_ends) KCTRY(launch_timed(c, KT_LASSM_ENDS, kc_lassm_ends_kernel, blocks(n_ends), tpb, 0, a, d_ends));
  const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (io.offsets_out) HIPCHK(hipMemcpyAsync(io.offsets_out, a.newoff, (n_ctgs + 1) * 8, back, c->stream));
  if (!dev) {
    if (total) HIPCHK(hipMemcpyAsync(io.seqs_out, d_out, total, hipMemcpyDeviceToHost, c->stream));
    if (io.ends && n_ends) HIPCHK(hipMemcpyAsync(io.ends, d_ends, n_ends * sizeof(kc_lassm_end), hipMemcpyDeviceToHost, c->stream));
  }
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
  if (p->min_mer_len < 4 || p->min_mer_len > p->max_mer_len || p->max_mer_len > KC_LASSM_MAX_MER_LEN || p->shift < 1 || p->shift > 64) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: mer lengths %u .. %u by %u outside 4 <= min <= max <= %d, 1 <= shift <= 64",
             p->min_mer_len, p->max_mer_len, p->shift, KC_LASSM_MAX_MER_LEN);
    return KC_ERR_INVALID_ARG;
  }
  if (p->max_walk_len < 1 || p->max_walk_len > KC_LASSM_MAX_WALK) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: max_walk_len %u outside 1 .. %d", p->max_walk_len, KC_LASSM_MAX_WALK);
    return KC_ERR_INVALID_ARG;
  }
  if (p->max_insert < 1 || p->max_insert > KC_INSERT_MAX) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: max_insert %u outside 1 .. %d", p->max_insert, KC_INSERT_MAX);
    return KC_ERR_INVALID_ARG;
  }
  if (p->min_qual > p->hi_qual || p->hi_qual > 93) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: qualities %u %u outside min_qual <= hi_qual <= 93", p->min_qual, p->hi_qual);
    return KC_ERR_INVALID_ARG;
  }
  if (p->min_viable < 1 || p->viable_permille > 1000) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: min_viable %u under 1 or viable_permille %u over 1000", p->min_viable,
             p->viable_permille);
    return KC_ERR_INVALID_ARG;
  }
  if (p->max_cands < 1 || p->max_cands > KC_LASSM_MAX_CANDS) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: max_cands %u outside 1 .. %u", p->max_cands, KC_LASSM_MAX_CANDS);
    return KC_ERR_INVALID_ARG;
  }
  if (p->flags) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: unknown flags 0x%x", p->flags);
    return KC_ERR_INVALID_ARG;
  }
  if (nreads & 1) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: %llu reads are no pairs (reads 2p and 2p + 1 are mates)",
             (unsigned long long)nreads);
    return KC_ERR_INVALID_ARG;
  }
  if (!c || (nreads && (!offsets || !pairs)) || (n_alns && !alns)) return KC_ERR_INVALID_ARG;
  if (on_device && (((uintptr_t)alns | (uintptr_t)pairs | (uintptr_t)ctgs | (uintptr_t)ends) & 15)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: a device record array is 16-byte aligned");
    return KC_ERR_INVALID_ARG;
  }
  if (on_device && (((uintptr_t)offsets | (uintptr_t)offsets_out) & 7)) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: device offsets are 8-byte aligned");
    return KC_ERR_INVALID_ARG;
  }
  if (!c->ai_ready) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: no contig index (kc_ctg_index_build)");
    return KC_ERR_STATE;
  }
  if (nreads >= (1ull << 30) || n_alns > 0xFFFFFFFFull) {
    snprintf(g_last_error, sizeof(g_last_error), "kc_local_assm: %llu reads, %llu records: an entry holds a read in 30 bits, a pair an index in 32",
             (unsigned long long)nreads, (unsigned long long)n_alns);
    return KC_ERR_CAPACITY;
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  LassmBufs b;
  const LassmIo io{bases, quals, offsets, nreads, alns, n_alns, pairs, ctgs, on_device, seqs_out, capacity, offsets_out, ends, nbytes_out, stats};
  const int rc = lassm_run(c, b, io, *p);
  if (rc) (void)hipStreamSynchronize(c->stream);
  b.release();
  return rc;
}
