// kc_api_call.hpp -- what the contig pass's entry points share on the host beyond kc_api_mem.hpp: the reads a host caller
// passes, the checks on reads, records and pairs, the two-level scan.  Part of kc_api.hip's translation unit, ahead of
// kc_api_sort.hpp.

static int no_ctg_index(const char *who) {
  return fail(KC_ERR_STATE, "%s: no contig index (kc_ctg_index_build)", who);
}

static int misaligned_records(const char *who) {
  return fail(KC_ERR_INVALID_ARG, "%s: a device record array is 16-byte aligned", who);
}

// the reads' nreads + 1 offsets: no reads, nothing to copy
static StagedIn<uint64_t> staged_offsets(const uint64_t *offsets, uint64_t nreads, bool dev) {
  return {offsets, dev, (size_t)(nreads + 1) * 8, nreads != 0};
}

// A host caller's read bytes in an allocation of their own, made once the lengths are checked so that no unchecked offset
// sizes it: the reads are the first `last` bytes.
static int upload_reads(kc_ctx *c, CallBufs &b, const uint8_t *bases, uint64_t last, const uint8_t **d_bases) {
  uint8_t *p;
  KCTRY(b.alloc(&p, last));
  HIPCHK(hipMemcpyAsync(p, bases, last, hipMemcpyHostToDevice, c->stream));
  *d_bases = p;
  return KC_OK;
}

// The verdict of a check kernel that leaves the lowest bad index in *d_bad (all ones: none).  fmt starts with %s for `who`
// and %llu for the index; `more` are what else it takes.
template <class... A> static int lowest_bad(kc_ctx *c, const uint64_t *d_bad, const char *fmt, const char *who, A... more) {
  uint64_t bad = ~0ull;
  KCTRY(read_back(c, &bad, d_bad, 1));
  if (bad == ~0ull) return KC_OK;
  return fail(KC_ERR_INVALID_ARG, fmt, who, (unsigned long long)bad, more...);
}

// ---- the checks on reads, records and pairs: nothing has been stored when one returns ----------------------------------
// The reads' lengths: offsets that do not decrease, at most ALIGN_MAX_READ_LEN apart.  d_als: ALS_COUNT zeroed words.  Gives
// the longest read and the last offset where asked (both 0 without reads); the two arrive with the verdict, in one wait.
static int check_read_lengths(kc_ctx *c, int kind, const char *who, const uint64_t *d_offs, uint64_t nreads, uint64_t *d_als,
                              uint64_t *max_len = nullptr, uint64_t *last = nullptr) {
  HIPCHK(hipMemsetAsync(d_als + ALS_BAD_READ, 0xFF, 8, c->stream));
  if (max_len) *max_len = 0;
  if (last) *last = 0;
  if (!nreads) return KC_OK;
  KCTRY(launch_timed(c, kind, kc_align_lengths_kernel, blocks_for(nreads), dim3(256), 0, d_offs, nreads, d_als));
  uint64_t h[ALS_COUNT];
  if (max_len)
    HIPCHK(hipMemcpyAsync(h, d_als, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  else
    HIPCHK(hipMemcpyAsync(h + ALS_BAD_READ, d_als + ALS_BAD_READ, 8, hipMemcpyDeviceToHost, c->stream));
  if (last) HIPCHK(hipMemcpyAsync(last, d_offs + nreads, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (h[ALS_BAD_READ] != ~0ull)
    return fail(KC_ERR_INVALID_ARG, "%s: read %llu is longer than %d bases, or its offsets decrease", who, (unsigned long long)h[ALS_BAD_READ],
                KC_ALIGN_MAX_READ_LEN);
  if (max_len) *max_len = h[ALS_MAX_LEN];
  return KC_OK;
}

// the validity pass over kc_gap_aln records and its verdict; a.st + DPS_BAD holds all ones
static int depth_check(kc_ctx *c, const DepthArgs &a, int kind, int use_reads, const char *who) {
  if (!a.n_alns) return KC_OK;
  KCTRY(launch_timed(c, kind, kc_depth_check_kernel, blocks_for(a.n_alns), dim3(256), 0, a, use_reads));
  return lowest_bad(c, a.st + DPS_BAD, "%s: record %llu is not a valid kc_gap_aln for this index%s", who, use_reads ? " and these reads" : "");
}

// ... of records against the kept index and these reads; d keeps what it is given beside (st; a caller's thresholds)
static int check_read_records(kc_ctx *c, DepthArgs &d, int kind, const char *who, const uint4 *alns, uint64_t n_alns, const uint64_t *offsets,
                              uint64_t nreads) {
  d.offs = c->ai.offs;
  d.n_ctgs = c->ai.n_ctgs;
  d.nbytes = (uint32_t)c->ai_nbytes;
  d.alns = alns;
  d.n_alns = n_alns;
  d.nreads = nreads;
  d.offsets = offsets;
  return depth_check(c, d, kind, 1, who);
}

// the pairs' records: a.pairs, a.alns, a.n_alns and a.nreads are set, a.st + LS_BAD_PAIR holds all ones
static int check_pairs(kc_ctx *c, const LassmArgs &a, uint64_t npairs, int kind, const char *who) {
  if (!npairs) return KC_OK;
  KCTRY(launch_timed(c, kind, kc_lassm_pair_check_kernel, blocks_for(npairs), dim3(256), 0, a));
  return lowest_bad(c, a.st + LS_BAD_PAIR, "%s: pair %llu names a record that is out of range, of another read or of kind KC_GAP_NONE", who);
}

// ---- the scan of more values than one workgroup takes ------------------------------------------------------------------
// values[n] become their exclusive prefix sums within tiles of LINK_SCAN_TILE, tile_base[] the tiles' bases, *total_out the sum
static int tiled_scan(kc_ctx *c, int kt_tile, int kt_scan, uint64_t *values, uint64_t n, uint64_t *tile_base, uint64_t *total_out) {
  const uint64_t tiles = (n + LINK_SCAN_TILE - 1) / LINK_SCAN_TILE;
  KCTRY(launch_timed(c, kt_tile, kc_link_tile_scan_kernel, dim3((unsigned)tiles), dim3(LINK_TILE), 0, values, n, tile_base));
  return launch_timed(c, kt_scan, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{tile_base}}, tiles, total_out);
}
