// kc_api_mem.hpp -- who owns the library's device and pinned memory, and how a HIP failure becomes a status.  Every
// allocation has an owner: a member of the context for memory that outlives a call, a CallBufs for memory that does not.
// The owners' destructors free, so no error return leaks and kc_destroy lists nothing.  Part of kc_api.hip's translation
// unit, ahead of kc_ctx; only this file (besides the arena probe) calls hipMalloc, hipFree, hipHostMalloc or hipHostFree.

struct kc_ctx;
static hipStream_t ctx_stream(const kc_ctx *c);  // under kc_ctx in kc_api.hip
static int ctx_device(const kc_ctx *c);

// an error return: the message kc_last_error() hands out, and the status it goes with
__attribute__((format(printf, 2, 3))) static int fail(int status, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
  return status;
}

static int hip_fail(hipError_t e, const char *what, const char *file, int line) {
  const char *base = strrchr(file, '/');
  return fail(e == hipErrorOutOfMemory ? KC_ERR_OUT_OF_MEMORY : KC_ERR_HIP, "%s failed at %s:%d: %s", what, base ? base + 1 : file, line,
              hipGetErrorString(e));
}

#define HIP_FAIL(e, what) hip_fail(e, what, __FILE__, __LINE__)

#define HIPCHK(call)                                    \
  do {                                                  \
    hipError_t e_ = (call);                             \
    if (e_ != hipSuccess) return HIP_FAIL(e_, #call);   \
  } while (0)

#define KCTRY(call)           \
  do {                        \
    const int rc_ = (call);   \
    if (rc_) return rc_;      \
  } while (0)

// ---- KC_DEBUG_FILL (kc_debug_fill.hpp) ---------------------------------------------------------------------------------
// A fresh allocation filled with the variable's byte: whatever the library reads before it has written it is then that
// byte, on every box and at every size, not what the allocator happened to hand out.  Unset: the getenv and nothing else.
// A device fill is complete on the device when this returns (the null stream is waited for), so that it is ordered
// ahead of any stream's work on the block.  Only reserve() below and the arena probe call it, on what they have just made.
static std::atomic<uint64_t> g_debug_filled{0};

static int debug_fill(void *p, size_t bytes, bool pinned) {
  const int fill = debug_fill_byte();
  if (fill < 0 || !p || !bytes) return KC_OK;
  if (pinned) {
    memset(p, fill, bytes);
  } else {
    HIPCHK(hipMemset(p, fill, bytes));
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  g_debug_filled += bytes;
  return KC_OK;
}

static dim3 blocks_for(uint64_t n, unsigned tpb = 256) { return dim3((unsigned)((n + tpb - 1) / tpb)); }

// ---- owners ------------------------------------------------------------------------------------------------------------
// One allocation of device (or pinned host) memory and its size.  It only ever grows: reserve() frees and allocates again
// when it is too small (the contents are lost then) and leaves {nullptr, 0} behind when the allocation fails.  Moving
// hands the allocation on and frees what the receiver held.  Growing with the contents kept is a fresh owner that is
// reserved, filled on the stream, waited for and swapped in: the old block goes with the fresh owner's scope, after its
// successor exists, and on any failure before the swap the old block is still the owner's (grow_table_nl, grow_results,
// grow_ovf2, bk_l2_reserve).
template <bool PINNED> struct Mem {
  uint8_t *p = nullptr;
  size_t cap = 0;  // bytes
  Mem() = default;
  Mem(Mem &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Mem &operator=(Mem &&o) noexcept {
    if (this != &o) {
      (void)release();
      swap(o);
    }
    return *this;
  }
  ~Mem() { (void)release(); }
  hipError_t release() {
    const hipError_t e = !p ? hipSuccess : PINNED ? hipHostFree(p) : hipFree(p);
    if (e == hipSuccess) p = nullptr, cap = 0;
    return e;
  }
  int reserve(size_t bytes) {
    if (bytes <= cap) return KC_OK;
    HIPCHK(release());
    HIPCHK(PINNED ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes));
    cap = bytes;
    return debug_fill(p, bytes, PINNED);
  }
  void swap(Mem &o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  // someone else has freed or taken the allocation (pick_fast_arena)
  void forget() { p = nullptr, cap = 0; }
  template <class T> T *as() const { return (T *)p; }
};
using DevBuf = Mem<false>;

// ... read as a T * wherever one is expected, so that kernel launches, copies and pointer arithmetic name the owner
template <class T, bool PINNED = false> struct Typed : Mem<PINNED> {
  operator T *() const { return (T *)this->p; }
  Typed &operator=(Mem<PINNED> &&o) {  // adopt an allocation made elsewhere (CallBufs::hand_over)
    Mem<PINNED>::operator=(std::move(o));
    return *this;
  }
};
template <class T> using Dev = Typed<T>;
template <class T> using Pin = Typed<T, true>;

// Bump carver over one scratch allocation, every piece aligned to 256 bytes.  A layout is a few lines that name its
// pieces; they run twice, on Carver{nullptr} for the size (`used`) and on Carver{base} for the pointers.
struct Carver {
  uint8_t *base;
  size_t used;
  template <class T> T *take(size_t n) {
    T *p = (T *)((uintptr_t)base + used);
    used += (n * sizeof(T) + 255) & ~size_t(255);
    return p;
  }
};

// ---- a call's device memory ------------------------------------------------------------------------------------------
// The allocations a call holds until it returns.
struct CallBufs {
  std::vector<DevBuf> held;
  // *p: `bytes` of device memory, or nullptr for none
  template <class T> int alloc(T **p, size_t bytes) {
    *p = nullptr;
    if (!bytes) return KC_OK;
    DevBuf d;
    KCTRY(d.reserve(bytes));
    *p = (T *)d.p;
    held.push_back(std::move(d));
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
  // `to` keeps p beyond the call, in place of what it held
  void hand_over(const void *p, DevBuf &to) {
    const auto it = std::find_if(held.begin(), held.end(), [&](const DevBuf &d) { return d.p == p; });
    if (it == held.end()) return;
    to = std::move(*it);
    held.erase(it);
  }
  void release() { held.clear(); }
};

// The frame of an entry point behind its host-side checks: body(CallBufs &) runs on the context's device; if it fails the
// stream is drained before the memory goes, so that no kernel still runs in it.
template <class F> static int call_with_bufs(kc_ctx *c, F &&body) {
  HIPCHK(hipSetDevice(ctx_device(c)));
  CallBufs b;
  const int rc = body(b);
  if (rc) (void)hipStreamSynchronize(ctx_stream(c));
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
    if (!dev && d && filled && bytes) HIPCHK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx_stream(c)));
    return KC_OK;
  }
};

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
    if (!dev && dst && d && bytes) HIPCHK(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, ctx_stream(c)));
    return KC_OK;
  }
};

// ---- reads back from the device ----------------------------------------------------------------------------------------
// n words to the host, and the stream drained: copies queued before it arrive with it
static int read_back(kc_ctx *c, uint64_t *h, const uint64_t *d, size_t n) {
  HIPCHK(hipMemcpyAsync(h, d, n * 8, hipMemcpyDeviceToHost, ctx_stream(c)));
  HIPCHK(hipStreamSynchronize(ctx_stream(c)));
  return KC_OK;
}

template <size_t N> static int read_back(kc_ctx *c, uint64_t (&h)[N], const uint64_t *d) { return read_back(c, h, d, N); }
