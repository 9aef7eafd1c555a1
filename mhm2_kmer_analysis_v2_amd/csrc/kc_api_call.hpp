// kc_api_call.hpp -- what the contig pass's entry points share on the host: the owner of a call's device memory and the
// call's frame, arrays that come from the host or the device, reads back from the device, the checks on reads, records
// and pairs, the two-level scan.  Part of kc_api.hip's translation unit, ahead of kc_api_sort.hpp.

static dim3 blocks_for(uint64_t n, unsigned tpb = 256) { return dim3((unsigned)((n + tpb - 1) / tpb)); }

static int no_ctg_index(const char *who) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: no contig index (kc_ctg_index_build)", who);
  return KC_ERR_STATE;
}

static int misaligned_records(const char *who) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: a device record array is 16-byte aligned", who);
  return KC_ERR_INVALID_ARG;
}

// ---- a call's device memory ------------------------------------------------------------------------------------------
// The allocations a call holds until it returns.
struct CallBufs {
  std::vector<void *> held;
  // *p: `bytes` of device memory, or nullptr for none
  template <class T> int alloc(T **p, size_t bytes) {
    *p = nullptr;
    if (!bytes) return KC_OK;
    HIPCHK(hipMalloc((void **)p, bytes));
    held.push_back(*p);
    return KC_OK;
  }
  // one allocation for a Carver layout: the layout runs on nullptr for the size and on the allocation for the pointers, so
  // it sets every pointer in either run and reads none that the first run left
  template <class L> int carve(L &&layout) {
    uint8_t *base;
    KCTRY(alloc(&base, layout((uint8_t *)nullptr)));
    layout(base);
    return KC_OK;
  }
  // the caller keeps p beyond the call
  void disown(void *p) { held.erase(std::remove(held.begin(), held.end(), p), held.end()); }
  void release() {
    for (void *p : held) (void)hipFree(p);
    held.clear();
  }
};

// The frame of an entry point behind its host-side checks: body(CallBufs &) runs on the context's device; if it fails the
// stream is drained before the memory goes, so that no kernel still runs in it.
template <class F> static int call_with_bufs(kc_ctx *c, F &&body) {
  HIPCHK(hipSetDevice(c->cfg.device));
  CallBufs b;
  const int rc = body(b);
  if (rc) (void)hipStreamSynchronize(c->stream);
  b.release();
  return rc;
}

// ---- arrays that are the host's or the device's ----------------------------------------------------------------------
// An input of `bytes` bytes as the kernels read it (d).  A device caller's array is read where it is; a host caller's gets
// room in the layout that calls reserve() and is copied there by upload() (`filled` false: there is nothing to copy).
template <class D> struct StagedIn {
  const void *src;
  bool dev;
  size_t bytes;
  bool filled;
  D *d;
  StagedIn(const void *src_, bool dev_, size_t bytes_, bool filled_ = true)
      : src(src_), dev(dev_), bytes(bytes_), filled(filled_), d(dev_ ? (D *)const_cast<void *>(src_) : nullptr) {}
  void reserve(Carver &m, bool want = true) {
    if (!dev && want) d = m.take<D>(bytes / sizeof(D));
  }
  int upload(kc_ctx *c) const {
    if (!dev && d && filled && bytes) HIPCHK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c->stream));
    return KC_OK;
  }
};

// the reads' nreads + 1 offsets: no reads, nothing to copy
static StagedIn<uint64_t> staged_offsets(const uint64_t *offsets, uint64_t nreads, bool dev) {
  return {offsets, dev, (size_t)(nreads + 1) * 8, nreads != 0};
}

// An optional output of `bytes` bytes as the kernels write it (d): nullptr where the caller passed none or the call's
// results do not fit.  A device caller's array is written where it is; a host caller's gets room in the layout that calls
// reserve() and is copied out by download(), which the caller's stream synchronisation completes.
template <class D> struct StagedOut {
  void *dst;
  bool dev;
  size_t bytes;
  D *d = nullptr;
  void reserve(Carver &m, bool fits = true) {
    if (dst && fits) d = dev ? (D *)dst : m.take<D>(bytes / sizeof(D));
  }
  int download(kc_ctx *c) const {
    if (!dev && dst && d && bytes) HIPCHK(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, c->stream));
    return KC_OK;
  }
};

// A host caller's read bytes in an allocation of their own, made once the lengths are checked so that no unchecked offset
// sizes it: the reads are the first `last` bytes.
static int upload_reads(kc_ctx *c, CallBufs &b, const uint8_t *bases, uint64_t last, const uint8_t **d_bases) {
  uint8_t *p;
  KCTRY(b.alloc(&p, last));
  HIPCHK(hipMemcpyAsync(p, bases, last, hipMemcpyHostToDevice, c->stream));
  *d_bases = p;
  return KC_OK;
}

// ---- reads back from the device ----------------------------------------------------------------------------------------
// n words to the host, and the stream drained: copies queued before it arrive with it
static int read_back(kc_ctx *c, uint64_t *h, const uint64_t *d, size_t n) {
  HIPCHK(hipMemcpyAsync(h, d, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

template <size_t N> static int read_back(kc_ctx *c, uint64_t (&h)[N], const uint64_t *d) { return read_back(c, h, d, N); }

// The verdict of a check kernel that leaves the lowest bad index in *d_bad (all ones: none).  fmt starts with %s for `who`
// and %llu for the index; `more` are what else it takes.
template <class... A> static int lowest_bad(kc_ctx *c, const uint64_t *d_bad, const char *fmt, const char *who, A... more) {
  uint64_t bad = ~0ull;
  KCTRY(read_back(c, &bad, d_bad, 1));
  if (bad == ~0ull) return KC_OK;
  snprintf(g_last_error, sizeof(g_last_error), fmt, who, (unsigned long long)bad, more...);
  return KC_ERR_INVALID_ARG;
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
  if (h[ALS_BAD_READ] != ~0ull) {
    snprintf(g_last_error, sizeof(g_last_error), "%s: read %llu is longer than %d bases, or its offsets decrease", who,
             (unsigned long long)h[ALS_BAD_READ], KC_ALIGN_MAX_READ_LEN);
    return KC_ERR_INVALID_ARG;
  }
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
