// kc_api_dedup.hpp -- kc_ctg_dedup (kernels in kc_dedup.hpp).  Part of kc_api.hip's translation unit, behind
// kc_api_asm.hpp; the check of the block is kc_align.hpp's, the scans kc_api_call.hpp's.

static_assert(sizeof(kc_dedup_params) == 32 && sizeof(kc_dedup_rec) == 32 && sizeof(kc_dedup_stats) == 128, "the header's layouts");
static_assert(KC_DEDUP_DUPLICATES_ONLY == DD_DUPLICATES_ONLY && KC_DEDUP_UNANCHORED == DD_UNANCHORED && KC_DEDUP_KEPT == DD_KEPT &&
                  KC_DEDUP_DUPLICATE == DD_DUPLICATE && KC_DEDUP_CONTAINED == DD_CONTAINED,
              "the header's constants are the kernels'");

struct DedupIo {
  const uint8_t *seqs;
  uint64_t nbytes;
  const uint64_t *offsets;
  uint64_t n_ctgs;
  const uint16_t *depths;
  int on_device;
  kc_dedup_rec *recs;
  uint8_t *seqs_out;
  uint64_t capacity;
  uint64_t *offsets_out;
  uint16_t *depths_out;
  uint64_t *n_out, *nbytes_out;
  kc_dedup_stats *stats;
};

template <int NL>
static int dedup_run(kc_ctx *c, CallBufs &b, const DedupIo &io, const kc_dedup_params &p) {
  const uint64_t n = io.n_ctgs, nbytes = io.nbytes;
  const bool dev = io.on_device != 0;
  const uint64_t tiles = (n + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  const uint64_t cap = next_pow2(std::max<uint64_t>(2 * n, 64));  // at most half full: a contig has one anchor
  const uint64_t max_cands = p.max_candidates ? p.max_candidates : 1ull << 26;
  DedupArgs a;
  memset(&a, 0, sizeof(a));
  uint64_t *d_ais;
  uint32_t *d_offs32;
  StagedIn<uint8_t> blk{io.seqs, dev, (size_t)nbytes, nbytes != 0};
  StagedIn<uint64_t> offs{io.offsets, dev, (size_t)(n + 1) * 8};
  size_t zeroed = 0;
  KCTRY(b.carve([&](uint8_t *base) {
    Carver m{base, 0};
    a.st = m.take<uint64_t>(DDS_COUNT);
    d_ais = m.take<uint64_t>(AIS_COUNT);
    a.slots = m.take<uint64_t>(cap);
    a.best = m.take<uint64_t>(n);
    a.absorbed = m.take<uint32_t>(n);
    a.wflag = m.take<uint8_t>(nbytes / DD_WIN_TPB + 1);
    zeroed = m.used;
    a.pick = m.take<uint64_t>(n);
    d_offs32 = m.take<uint32_t>(n + 1);
    a.akey = m.take<uint64_t>(n * NL);
    a.ainfo = m.take<uint2>(n);
    a.next = m.take<uint32_t>(n);
    a.klen = m.take<uint64_t>(n);
    a.kflag = m.take<uint64_t>(n);
    a.lbase = m.take<uint64_t>(tiles);
    a.fbase = m.take<uint64_t>(tiles);
    blk.reserve(m);
    offs.reserve(m);
    return m.used;
  }));
  KCTRY(blk.upload(c));
  KCTRY(offs.upload(c));
  HIPCHK(hipMemsetAsync(a.st, 0, zeroed, c->stream));
  if (n) HIPCHK(hipMemsetAsync(a.pick, 0xFF, n * 8, c->stream));
  // ---- the check: nothing is stored through the caller's pointers before its verdict
  const dim3 tpb(DD_TPB), per_window = blocks_for(nbytes, DD_WIN_TPB * DD_WIN_ITEMS);
  KCTRY(launch_timed(c, KT_DEDUP_CHECK, kc_align_check_kernel, blocks_for(std::max(nbytes, n + 1)), dim3(256), 0, (const uint8_t *)blk.d, nbytes,
                     (const uint64_t *)offs.d, n, d_offs32, d_ais));
  uint64_t ha[AIS_COUNT];
  KCTRY(read_back(c, ha, d_ais));
  if (ha[AIS_BAD_BASE]) return fail(KC_ERR_BAD_BASE, "kc_ctg_dedup: a byte outside ACGTN and '_' in the block");
  if (ha[AIS_BAD_OFFSETS] || ha[AIS_SEPARATORS] != n)
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_dedup: the offsets of %llu contigs do not match the block's %llu separators", (unsigned long long)n,
                (unsigned long long)ha[AIS_SEPARATORS]);
  a.seqs = blk.d;
  a.offs = d_offs32;
  a.nbytes = (uint32_t)nbytes;
  a.n = (uint32_t)n;
  a.k = c->k;
  a.flags = p.flags;
  a.max_mm = p.max_mismatches;
  a.mask = cap - 1;
  uint64_t h[DDS_COUNT];
  memset(h, 0, sizeof(h));
  if (n) {
    // ---- anchors, their table, and the windows that meet one
    KCTRY(launch_timed(c, KT_DEDUP_ANCHOR, kc_dedup_anchor_kernel<NL>, blocks_for(n * 64, DD_TPB), tpb, 0, a));
    KCTRY(launch_timed(c, KT_DEDUP_LINK, kc_dedup_link_kernel<NL>, blocks_for(n, DD_TPB), tpb, 0, a));
    KCTRY(launch_timed(c, KT_DEDUP_COUNT, kc_dedup_windows_kernel<NL, false>, per_window, dim3(DD_WIN_TPB), 0, a));
    KCTRY(read_back(c, h, a.st));
    a.n_cands = h[DDS_CANDS];
    a.n_short = h[DDS_CANDS] - h[DDS_LONG];
    if (a.n_cands > max_cands)
      return fail(KC_ERR_CAPACITY, "kc_ctg_dedup: %llu candidates, max_candidates is %llu", (unsigned long long)a.n_cands,
                  (unsigned long long)max_cands);
    if (a.n_cands) {
      KCTRY(b.alloc(&a.cands, a.n_cands * sizeof(uint4)));
      KCTRY(launch_timed(c, KT_DEDUP_WRITE, kc_dedup_windows_kernel<NL, true>, blocks_for(nbytes, DD_WIN_TPB), dim3(DD_WIN_TPB), 0, a));
      // ---- the comparison: a wave a short candidate, a wave a segment of a long one, 65535 long ones a launch
      if (a.n_short) KCTRY(launch_timed(c, KT_DEDUP_VERIFY, kc_dedup_verify_kernel<false>, blocks_for(a.n_short * 64, DD_TPB), tpb, 0, a));
      const uint64_t n_long = h[DDS_LONG], segs = (h[DDS_MAX_LONG] + 15 + DD_SEG - 1) / DD_SEG;
      for (a.row0 = 0; a.row0 < n_long; a.row0 += 65535) {
        const dim3 grid(blocks_for(segs * 64, DD_TPB).x, (unsigned)std::min<uint64_t>(n_long - a.row0, 65535));
        KCTRY(launch_timed(c, KT_DEDUP_VERIFY_LONG, kc_dedup_verify_kernel<true>, grid, tpb, 0, a));
      }
      a.row0 = 0;
      // ---- per contig: the container of highest rank, then its smallest (j, o)
      KCTRY(launch_timed(c, KT_DEDUP_BEST, kc_dedup_best_kernel, blocks_for(a.n_cands, DD_TPB), tpb, 0, a));
      KCTRY(launch_timed(c, KT_DEDUP_PICK, kc_dedup_pick_kernel, blocks_for(a.n_cands, DD_TPB), tpb, 0, a));
    }
    KCTRY(launch_timed(c, KT_DEDUP_STATUS, kc_dedup_status_kernel, blocks_for(n, DD_TPB), tpb, 0, a));
    KCTRY(tiled_scan(c, KT_DEDUP_TILE_SCAN, KT_DEDUP_SCAN, a.klen, n, a.lbase, a.st + DDS_SCAN_BYTES));
    KCTRY(tiled_scan(c, KT_DEDUP_TILE_SCAN, KT_DEDUP_SCAN, a.kflag, n, a.fbase, a.st + DDS_SCAN_KEPT));
    KCTRY(read_back(c, h, a.st));
    if (h[DDS_SCAN_BYTES] != h[DDS_KEPT_BYTES] || h[DDS_SCAN_KEPT] != h[DDS_KEPT] || h[DDS_KEPT] + h[DDS_DUP] + h[DDS_CONT] != n)
      return fail(KC_ERR_STATE, "kc_ctg_dedup: the scans give %llu bytes of %llu contigs, the sums %llu of %llu", (unsigned long long)h[DDS_SCAN_BYTES],
                  (unsigned long long)h[DDS_SCAN_KEPT], (unsigned long long)h[DDS_KEPT_BYTES], (unsigned long long)h[DDS_KEPT]);
  }
  const uint64_t n_kept = h[DDS_KEPT], total = h[DDS_KEPT_BYTES];
  kc_dedup_stats s;
  memset(&s, 0, sizeof(s));
  s.contigs = n;
  s.bases = nbytes - n;
  s.anchored = h[DDS_ANCHORED];
  s.unanchored = n - h[DDS_ANCHORED];
  s.windows = h[DDS_WINDOWS];
  s.window_hits = h[DDS_HITS];
  s.candidates = h[DDS_CANDS];
  s.verified = h[DDS_VERIFIED];
  s.duplicates = h[DDS_DUP];
  s.contained = h[DDS_CONT];
  s.kept = n_kept;
  s.kept_bases = total - n_kept;
  s.removed_bases = h[DDS_REMOVED_BASES];
  s.longest_removed = h[DDS_LONGEST_REMOVED];
  const bool fits = io.seqs_out && io.capacity >= total;
  if (fits) {
    StagedOut<uint8_t> seqs{io.seqs_out, dev, (size_t)total};
    StagedOut<uint64_t> offsets{io.offsets_out, dev, (size_t)(n_kept + 1) * 8};
    StagedOut<uint4> recs{io.recs, dev, (size_t)n * sizeof(kc_dedup_rec)};
    StagedOut<uint16_t> depths{io.depths ? io.depths_out : nullptr, dev, (size_t)total * 2};
    StagedIn<uint16_t> din{io.depths, dev, (size_t)nbytes * 2, nbytes != 0};
    KCTRY(b.carve([&](uint8_t *base) {
      Carver m{base, 0};
      a.noff = m.take<uint32_t>(n_kept + 1);
      a.gsrc = m.take<uint32_t>(n_kept + 1);
      seqs.reserve(m);
      offsets.reserve(m);
      recs.reserve(m);
      depths.reserve(m);
      din.reserve(m, depths.dst != nullptr);
      return m.used;
    }));
    if (depths.dst) KCTRY(din.upload(c));
    a.recs = recs.d;
    a.offsets_out = offsets.d;
    a.n_kept = (uint32_t)n_kept;
    a.total = (uint32_t)total;
    if (n) {
      KCTRY(launch_timed(c, KT_DEDUP_RECORDS, kc_dedup_records_kernel, blocks_for(n, DD_TPB), tpb, 0, a));
      DedupCopy g{blk.d, seqs.d, a.noff, a.gsrc, a.n_kept, a.total, a.nbytes};
      const uint64_t chunks = (total + 15 + 15) / 16;  // a misaligned array's first chunk is partial
      KCTRY(launch_timed(c, KT_DEDUP_GATHER, kc_dedup_gather_kernel<1>, blocks_for(chunks, DD_TPB), tpb, 0, g));
      if (depths.d) {
        g.src = (const uint8_t *)din.d;
        g.dst = (uint8_t *)depths.d;
        KCTRY(launch_timed(c, KT_DEDUP_GATHER_DEPTHS, kc_dedup_gather_kernel<2>, blocks_for((2 * total + 15 + 15) / 16, DD_TPB), tpb, 0, g));
      }
    } else if (offsets.d)
      HIPCHK(hipMemsetAsync(offsets.d, 0, 8, c->stream));
    KCTRY(seqs.download(c));
    KCTRY(offsets.download(c));
    KCTRY(recs.download(c));
    KCTRY(depths.download(c));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  *io.n_out = n_kept;
  *io.nbytes_out = total;
  if (io.stats) *io.stats = s;
  if (io.seqs_out && !fits)
    return fail(KC_ERR_CAPACITY, "kc_ctg_dedup: %llu bytes, the array holds %llu", (unsigned long long)total, (unsigned long long)io.capacity);
  return KC_OK;
}

extern "C" int kc_ctg_dedup(kc_ctx *c, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, const uint16_t *depths,
                            int on_device, const kc_dedup_params *p, kc_dedup_rec *recs, uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out,
                            uint16_t *depths_out, uint64_t *n_out, uint64_t *nbytes_out, kc_dedup_stats *stats) {
  // the ranges come before the context so that they can be checked where there is no device
  if (!p || !n_out || !nbytes_out) return fail(KC_ERR_INVALID_ARG, "kc_ctg_dedup: %s is NULL", !p ? "params" : !n_out ? "n_out" : "nbytes_out");
  if (p->flags & ~KC_DEDUP_DUPLICATES_ONLY) return fail(KC_ERR_INVALID_ARG, "kc_ctg_dedup: unknown flags 0x%x", p->flags & ~KC_DEDUP_DUPLICATES_ONLY);
  for (int i = 0; i < 4; i++)
    if (p->reserved[i]) return fail(KC_ERR_INVALID_ARG, "kc_ctg_dedup: reserved[%d] is %u, not zero", i, p->reserved[i]);
  if (!c) return KC_ERR_INVALID_ARG;
  KCTRY(asm_block_args("kc_ctg_dedup", seqs, nbytes, offsets, n_ctgs));
  if (on_device && (((uintptr_t)recs) & 15)) return misaligned_records("kc_ctg_dedup");
  if (on_device && ((((uintptr_t)offsets | (uintptr_t)offsets_out) & 7) || (((uintptr_t)depths | (uintptr_t)depths_out) & 1)))
    return fail(KC_ERR_INVALID_ARG, "kc_ctg_dedup: device offsets are 8-byte aligned, depths 2-byte");
  const DedupIo io{seqs, nbytes, offsets, n_ctgs, depths, on_device, recs, seqs_out, capacity, offsets_out, depths_out, n_out, nbytes_out, stats};
  return call_with_bufs(c, [&](CallBufs &b) { return with_nl(c, [&](auto nl) { return dedup_run<nl>(c, b, io, *p); }); });
}
