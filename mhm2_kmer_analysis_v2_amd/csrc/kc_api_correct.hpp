// kc_api_correct.hpp -- kc_correct_reads (kernels in kc_correct.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_kdepth.hpp; the index is kc_lookup's (ensure_index), the track pass kc_seq_kmer_depths'.
//
// The entry point is declared in include/kcount_mi355_correct.h, inside that header's extern "C" block, and defined here
// without a linkage specifier of its own, as kc_api_kdepth.hpp does: tests/test_poisoned_scratch_coverage.py finds entry points
// by the specifier's text and holds a closed list.  tests/test_entry_point_coverage_correct.py reads the second header instead.

static_assert(sizeof(kc_correct_params) == 32 && sizeof(kc_correct_rec) == 16 && sizeof(kc_correct_fix) == 16 && sizeof(kc_correct_stats) == 64,
              "the header's layouts");
static_assert(offsetof(kc_correct_rec, corrected) == 8 && offsetof(kc_correct_rec, flags) == 10 && offsetof(kc_correct_fix, old_base) == 8 &&
                  offsetof(kc_correct_fix, round) == 10 && offsetof(kc_correct_fix, side) == 11 && offsetof(kc_correct_fix, score) == 12,
              "kc_correct_records_kernel and kc_correct_apply_kernel write these");
static_assert(KC_CORRECT_UNANCHORED == CRF_UNANCHORED && KC_CORRECT_SHORT_RUN == CRF_SHORT_RUN && KC_CORRECT_THIN == CRF_THIN &&
                  KC_CORRECT_QUAL_GATED == CRF_QUAL_GATED && KC_CORRECT_NO_GAIN == CRF_NO_GAIN && KC_CORRECT_AMBIGUOUS == CRF_AMBIGUOUS,
              "the header's constants are the kernels'");

struct CorrectIo {
  const uint8_t *bases, *quals;
  uint64_t nbytes;
  const uint64_t *offsets;
  uint64_t nseqs;
  int on_device;
  uint8_t *out;
  kc_correct_rec *recs;
  kc_correct_fix *fixes;
  uint64_t fix_capacity;
  kc_correct_stats *stats;
};

// the fixes of one round, in the call's memory
struct CorrectRound {
  const uint4 *fixes;
  uint64_t n;
};

template <int NL>
static int correct_run(kc_ctx *c, CallBufs &b, const CorrectIo &io, const kc_correct_params &p) {
  const uint64_t n = io.nseqs, nbytes = io.nbytes;
  const bool dev = io.on_device != 0, gate = io.quals && p.max_qual;
  // a device caller's out is the working text unless the call can still fail on the fixes' capacity
  const bool own_text = !dev || io.fixes;
  KCTRY(ensure_index<NL>(c));
  const uint64_t lanes_n = (nbytes + KT_RUN - 1) / KT_RUN;
  const dim3 tpb(KT_TPB), lanes = blocks_for(lanes_n, KT_TPB), per_seq = blocks_for(n, CR_TPB);
  KtrackArgs t;
  memset(&t, 0, sizeof(t));
  CorrectArgs a;
  memset(&a, 0, sizeof(a));
  StagedIn<uint8_t> quals{io.quals, dev, (size_t)nbytes};
  StagedIn<uint64_t> offs{io.offsets, dev, (size_t)(n + 1) * 8};
  StagedOut<uint4> recs{io.recs, dev, (size_t)n * sizeof(kc_correct_rec)};
  uint64_t *totals = nullptr;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    t.st = m.take<uint64_t>(KTS_COUNT);
    totals = m.take<uint64_t>(1);
    a.weak = m.take<uint32_t>(n);
    a.why_sites = m.take<uint32_t>(n);
    a.why_eval = m.take<uint32_t>(n);
    a.corrected = m.take<uint32_t>(n);
    a.weak_before = m.take<uint32_t>(n);
    a.lane_sites = m.take<uint8_t>(lanes_n);
    a.wg_sites = m.take<uint64_t>(lanes.x);
    t.track = m.take<uint16_t>(nbytes);
    a.text = own_text ? m.take<uint8_t>(nbytes) : io.out;
    quals.reserve(m, gate);
    offs.reserve(m);
    recs.reserve(m);
    return m.used;
  }));
  KCTRY(offs.upload(c));
  HIPCHK(hipMemsetAsync(t.st, 0xFF, 2 * 8, c->stream));  // KTS_BAD, KTS_LONG: the lowest index, all ones for none
  HIPCHK(hipMemsetAsync(t.st + 2, 0, (KTS_COUNT - 2) * 8, c->stream));
  // ---- the check: nothing is stored through the caller's pointers before its verdict
  KCTRY(launch_timed(c, KT_CORRECT_OFFSETS, kc_ktrack_offsets_kernel, blocks_for(n, KT_TPB), tpb, 0, (const uint64_t *)offs.d, n, nbytes, t.st));
  uint64_t h[KTS_COUNT];
  KCTRY(read_back(c, h, t.st));
  if (h[KTS_BAD] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: the offsets decrease behind sequence %llu", (unsigned long long)h[KTS_BAD]);
  if (h[KTS_ENDS])
    return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: the offsets of %llu sequences do not %s", (unsigned long long)n,
                (h[KTS_ENDS] & 1) ? "start at 0" : "end at nbytes");
  if (h[KTS_LONG] != ~0ull)
    return fail(KC_ERR_CAPACITY, "kc_correct_reads: sequence %llu has 2^32 bytes or more", (unsigned long long)h[KTS_LONG]);
  HIPCHK(hipMemcpyAsync(a.text, io.bases, nbytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  if (gate) KCTRY(quals.upload(c));
  HIPCHK(hipMemsetAsync(a.corrected, 0, n * 4, c->stream));
  HIPCHK(hipMemsetAsync(a.why_eval, 0, n * 4, c->stream));
  t.seqs = a.text;
  t.nbytes = a.nbytes = nbytes;
  t.offs = a.offs = offs.d;
  t.n = a.n = (uint32_t)n;
  t.k = a.k = c->k;
  t.solid = a.solid = std::max(p.min_count, 1u);
  t.index = a.index = c->d_index;
  t.mask = a.mask = c->index_cap - 1;
  t.keys = a.keys = c->d_out_keys;
  t.counts = a.counts = c->d_out_counts;
  a.track = t.track;
  a.quals = gate ? quals.d : nullptr;
  a.min_gain = p.min_gain;
  a.min_windows = p.min_windows;
  a.max_qual = p.max_qual;
  a.qual_offset = c->cfg.qual_offset;
  a.recs = recs.d;
  uint32_t *const why_sites = a.why_sites;
  // the track of the current text, the weak windows per sequence and the sites' counts; h: the track's totals, *sites: the sites
  auto survey = [&](bool with_reasons, uint64_t *sites) -> int {
    HIPCHK(hipMemsetAsync(t.st, 0, KTS_COUNT * 8, c->stream));
    HIPCHK(hipMemsetAsync(a.weak, 0, n * 4, c->stream));
    a.why_sites = with_reasons ? why_sites : nullptr;
    if (with_reasons) HIPCHK(hipMemsetAsync(why_sites, 0, n * 4, c->stream));
    KCTRY(launch_timed(c, KT_CORRECT_TRACK, kc_ktrack_windows_kernel<NL, false>, lanes, tpb, 0, t));
    KCTRY(launch_timed(c, KT_CORRECT_SITES_COUNT, kc_correct_sites_kernel<false>, lanes, tpb, 0, a));
    KCTRY(launch_timed(c, KT_CORRECT_SITES_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.wg_sites}}, (uint64_t)lanes.x, totals));
    HIPCHK(hipMemcpyAsync(sites, totals, 8, hipMemcpyDeviceToHost, c->stream));
    return read_back(c, h, t.st);
  };
  std::vector<CorrectRound> done;
  uint64_t weak_before = 0, evaluated = 0, accepted = 0, rounds = 0;
  bool final_track = false;  // the last survey is of the text as it is now
  for (uint32_t r = 1; r <= p.rounds; r++) {
    uint64_t n_sites = 0;
    KCTRY(survey(true, &n_sites));
    rounds = r;
    final_track = true;
    if (r == 1) {
      weak_before = h[KTS_WINDOWS] - h[KTS_SOLID];
      HIPCHK(hipMemcpyAsync(a.weak_before, a.weak, n * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(hipMemsetAsync(a.why_eval, 0, n * 4, c->stream));
    if (!n_sites) break;
    uint8_t *round_mem;
    KCTRY(b.alloc(&round_mem, [&] {
      Carver m{nullptr, 0};
      m.take<uint4>(n_sites), m.take<uint2>(n_sites), m.take<uint64_t>(n_sites), m.take<uint4>(n_sites);
      return m.used;
    }()));
    Carver m{round_mem, 0};
    a.sites = m.take<uint4>(n_sites);
    a.verdicts = m.take<uint2>(n_sites);
    a.slots = m.take<uint64_t>(n_sites);
    a.fixes = m.take<uint4>(n_sites);
    a.n_sites = n_sites;
    a.round = r;
    a.why_sites = why_sites;
    KCTRY(launch_timed(c, KT_CORRECT_SITES_WRITE, kc_correct_sites_kernel<true>, lanes, tpb, 0, a));
    KCTRY(launch_timed(c, KT_CORRECT_EVAL, kc_correct_eval_kernel<NL>, blocks_for(n_sites, CR_WAVES), dim3(CR_TPB), 0, a));
    KCTRY(launch_timed(c, KT_CORRECT_ACCEPT_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.slots}}, n_sites, totals));
    KCTRY(launch_timed(c, KT_CORRECT_APPLY, kc_correct_apply_kernel, blocks_for(n_sites, CR_TPB), dim3(CR_TPB), 0, a));
    uint64_t got = 0;
    KCTRY(read_back(c, &got, totals, 1));
    evaluated += n_sites;
    if (!got) break;
    accepted += got;
    done.push_back({a.fixes, got});
    final_track = false;
  }
  if (io.fixes && accepted > io.fix_capacity)
    return fail(KC_ERR_CAPACITY, "kc_correct_reads: %llu fixes, room for %llu", (unsigned long long)accepted, (unsigned long long)io.fix_capacity);
  if (!final_track) {
    uint64_t n_sites = 0;
    KCTRY(survey(false, &n_sites));
  }
  a.why_sites = why_sites;
  if (a.recs) KCTRY(launch_timed(c, KT_CORRECT_RECORDS, kc_correct_records_kernel, per_seq, dim3(CR_TPB), 0, a));
  // ---- out: from here on the caller's arrays are written
  if (own_text) HIPCHK(hipMemcpyAsync(io.out, a.text, nbytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  if (io.fixes) {
    uint64_t at = 0;
    for (const CorrectRound &r : done) {
      HIPCHK(hipMemcpyAsync(io.fixes + at, r.fixes, r.n * sizeof(kc_correct_fix), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
      at += r.n;
    }
  }
  KCTRY(recs.download(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (io.stats) {
    kc_correct_stats s;
    memset(&s, 0, sizeof(s));
    s.seqs = n;
    s.bytes = nbytes;
    s.windows = h[KTS_WINDOWS];
    s.weak_before = weak_before;
    s.weak_after = h[KTS_WINDOWS] - h[KTS_SOLID];
    s.sites = evaluated;
    s.accepted = accepted;
    s.rounds = rounds;
    *io.stats = s;
  }
  return KC_OK;
}

// no sequences or no bytes: out = bases, zero records and stats
static int correct_nothing(kc_ctx *c, const CorrectIo &io) {
  if (io.on_device) {
    if (io.nbytes) HIPCHK(hipMemcpyAsync(io.out, io.bases, io.nbytes, hipMemcpyDeviceToDevice, c->stream));
    if (io.recs && io.nseqs) HIPCHK(hipMemsetAsync(io.recs, 0, io.nseqs * sizeof(kc_correct_rec), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    if (io.nbytes) memcpy(io.out, io.bases, io.nbytes);
    if (io.recs && io.nseqs) memset(io.recs, 0, io.nseqs * sizeof(kc_correct_rec));
  }
  if (io.stats) memset(io.stats, 0, sizeof(*io.stats));
  return KC_OK;
}

int kc_correct_reads(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets, uint64_t nseqs,
                     int on_device, const kc_correct_params *p, uint8_t *out, kc_correct_rec *recs, kc_correct_fix *fixes, uint64_t fix_capacity,
                     kc_correct_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !offsets) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: %s is NULL", !p ? "params" : "offsets");
  if ((!bases || !out) && nbytes)
    return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: %s is NULL with %llu bytes", !bases ? "bases" : "out", (unsigned long long)nbytes);
  if (p->min_count > 65535u) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: min_count is %u, at most 65535", p->min_count);
  if (!p->min_gain) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: min_gain is 0, at least 1");
  if (p->rounds < 1 || p->rounds > KC_CORRECT_MAX_ROUNDS)
    return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: rounds is %u, 1 to %d", p->rounds, KC_CORRECT_MAX_ROUNDS);
  if (p->max_qual > 255u) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: max_qual is %u, at most 255", p->max_qual);
  if (p->flags) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: unknown flags 0x%x", p->flags);
  for (int i = 0; i < 2; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (nbytes && (bases < out ? (uint64_t)(out - bases) : (uint64_t)(bases - out)) < nbytes)
    return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: out overlaps bases");
  if (!c) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: ctx is NULL");
  if (nseqs >= (1ull << 32)) return fail(KC_ERR_CAPACITY, "kc_correct_reads: %llu sequences, at most 2^32 - 1", (unsigned long long)nseqs);
  if (on_device && ((((uintptr_t)recs) | ((uintptr_t)fixes)) & 15)) return misaligned_records("kc_correct_reads");
  if (on_device && (((uintptr_t)offsets) & 7)) return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: device offsets are 8-byte aligned");
  if (c->cfg.rank_n > 1)
    return fail(KC_ERR_INVALID_ARG, "kc_correct_reads: rank_n is %d; a k-mer of another rank looks absent, so reads are corrected on one rank only",
                c->cfg.rank_n);
  if (!c->finalized) return fail(KC_ERR_STATE, "kc_correct_reads: no results (kc_finalize)");
  const CorrectIo io{bases, quals, nbytes, offsets, nseqs, on_device, out, recs, fixes, fix_capacity, stats};
  return call_with_bufs(c, [&](CallBufs &b) {
    if (!nseqs || !nbytes) return correct_nothing(c, io);
    return with_nl(c, [&](auto nl) { return correct_run<nl>(c, b, io, *p); });
  });
}
