// kc_api_frontend.hpp -- host side of the read front end in front of the k-mer counter: the FASTQ parsers (host and
// device, kc_fastq.hpp), the overlap merge of pairs (kc_merge.hpp) and the adapter trim (kc_trim.hpp).  Part of
// kc_api.hip's translation unit: it is included there, after the context and its helpers, and nowhere else.
#pragma once
// ---- FASTQ front end (host only) -----------------------------------------------------------------------------------
// base codes of PackedRead (packed_reads.cpp:99-124): 255 = the reference DIEs
static void fq_code_table(uint8_t code[256]) {
  memset(code, 255, 256);
  const char *acgt = "ACGT";
  for (int i = 0; i < 4; i++) code[(uint8_t)acgt[i]] = code[(uint8_t)(acgt[i] | 0x20)] = (uint8_t)i;
  code[(uint8_t)'N'] = code[(uint8_t)'n'] = 4;
  for (const char *p = "URYKMSWBDHV"; *p; p++) code[(uint8_t)*p] = 4;
}

// one FASTQ record of text[pos, len): 1 with [sb, sb + *sl) the sequence and [qb, qb + *sl) the qualities, 0 at the end,
// KC_ERR_INVALID_ARG for a malformed record (kc_last_error names the line)
struct FqCursor {
  const char *text;
  uint64_t len, pos, line_no;
};

static int fq_next(FqCursor &f, uint64_t *sb, uint64_t *qb, uint64_t *sl) {
  auto next_line = [&](uint64_t &b, uint64_t &e) -> bool {  // [b, e): the line without its end and trailing white space
    if (f.pos >= f.len) return false;
    b = f.pos;
    while (f.pos < f.len && f.text[f.pos] != '\n') f.pos++;
    e = f.pos;
    if (f.pos < f.len) f.pos++;
    while (e > b && (f.text[e - 1] == '\r' || f.text[e - 1] == ' ' || f.text[e - 1] == '\t')) e--;
    f.line_no++;
    return true;
  };
  const char *text = f.text;
  const uint64_t len = f.len;
  uint64_t b0, e0, b1, e1, b2, e2, b3, e3;
  if (!next_line(b0, e0)) return 0;
  if (e0 == b0 && f.pos >= len) return 0;  // a final empty line
  if (!next_line(b1, e1) || !next_line(b2, e2) || !next_line(b3, e3))
    return fail(KC_ERR_INVALID_ARG, "FASTQ ends inside the record that starts at line %llu", (unsigned long long)(f.line_no - (f.line_no - 1) % 4));
  if (e0 == b0 || text[b0] != '@')
    return fail(KC_ERR_INVALID_ARG, "Invalid FASTQ: expected read name (@) at line %llu", (unsigned long long)(f.line_no - 3));
  if (e2 == b2 || text[b2] != '+') return fail(KC_ERR_INVALID_ARG, "Invalid FASTQ: expected '+' at line %llu", (unsigned long long)(f.line_no - 1));
  if (e1 - b1 != e3 - b3)
    return fail(KC_ERR_INVALID_ARG, "Invalid FASTQ: sequence length %llu != %llu quals length at line %llu", (unsigned long long)(e1 - b1),
                (unsigned long long)(e3 - b3), (unsigned long long)(f.line_no - 2));
  *sb = b1;
  *qb = b3;
  *sl = e1 - b1;
  return 1;
}

extern "C" int kc_fastq_to_packed(const char *text, uint64_t len, int qual_offset, uint8_t *packed, uint64_t packed_capacity,
                                  uint64_t *offsets, uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes) {
  if ((len && !text) || !nreads || !nbytes) return KC_ERR_INVALID_ARG;
  uint8_t code[256];
  fq_code_table(code);
  uint64_t nr = 0, nb = 0;
  bool fits = true;
  FqCursor f{text, len, 0, 0};
  if (offsets && reads_capacity + 1 > 0) offsets[0] = 0;
  for (;;) {
    uint64_t b1, b3, sl;
    const int r = fq_next(f, &b1, &b3, &sl);
    if (r < 0) return r;
    if (r == 0) break;
    const bool room = fits && packed && offsets && nr < reads_capacity && nb + sl <= packed_capacity;
    for (uint64_t i = 0; i < sl; i++) {
      const uint8_t cb = code[(uint8_t)text[b1 + i]];
      if (cb == 255)
        return fail(KC_ERR_BAD_BASE, "Illegal char in comp nucleotide (int=%d) at line %llu", (int)(uint8_t)text[b1 + i],
                    (unsigned long long)(f.line_no - 2));
      if (room) {
        int q = (int)(uint8_t)text[b3 + i] - qual_offset;
        if (q > 31) q = 31;
        packed[nb + i] = (uint8_t)(cb | ((uint8_t)q << 3));  // like the reference's (unsigned char)std::min(q, 31) << 3
      }
    }
    if (!room) fits = false;
    nb += sl;
    nr++;
    if (room) offsets[nr] = nb;
  }
  *nreads = nr;
  *nbytes = nb;
  if (!fits && (nr || nb))
    return fail(KC_ERR_CAPACITY, "%llu reads with %llu bases do not fit the arrays", (unsigned long long)nr, (unsigned long long)nb);
  return KC_OK;
}

extern "C" int kc_fastq_pairs(const char *text1, uint64_t len1, const char *text2, uint64_t len2, uint8_t *bases, uint8_t *quals,
                              uint64_t capacity, uint64_t *offsets, uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes) {
  if ((len1 && !text1) || (len2 && !text2) || !nreads || !nbytes) return KC_ERR_INVALID_ARG;
  uint8_t code[256];
  fq_code_table(code);
  FqCursor f[2] = {{text1, len1, 0, 0}, {text2, len2, 0, 0}};
  const bool two = text2 != nullptr;
  uint64_t nr = 0, nb = 0;
  bool fits = true;
  if (offsets && reads_capacity + 1 > 0) offsets[0] = 0;
  for (;;) {
    FqCursor &fc = f[two ? (nr & 1) : 0];
    uint64_t b1, b3, sl;
    const int r = fq_next(fc, &b1, &b3, &sl);
    if (r < 0) return r;
    if (r == 0) {
      if (two && (nr & 1))
        return fail(KC_ERR_INVALID_ARG, "the second file ends after %llu records, the first has more", (unsigned long long)(nr / 2));
      if (two) {  // the first file ended: the second must end too
        uint64_t x, y, z;
        const int r2 = fq_next(f[1], &x, &y, &z);
        if (r2 < 0) return r2;
        if (r2 > 0) return fail(KC_ERR_INVALID_ARG, "the first file ends after %llu records, the second has more", (unsigned long long)(nr / 2));
      }
      break;
    }
    const bool room = fits && bases && quals && offsets && nr < reads_capacity && nb + sl <= capacity;
    for (uint64_t i = 0; i < sl; i++) {
      if (code[(uint8_t)fc.text[b1 + i]] == 255)
        return fail(KC_ERR_BAD_BASE, "Illegal char in comp nucleotide (int=%d) at line %llu of file %d", (int)(uint8_t)fc.text[b1 + i],
                    (unsigned long long)(fc.line_no - 2), two ? (int)(nr & 1) + 1 : 1);
    }
    if (room) {
      memcpy(bases + nb, fc.text + b1, sl);
      memcpy(quals + nb, fc.text + b3, sl);
    } else {
      fits = false;
    }
    nb += sl;
    nr++;
    if (room) offsets[nr] = nb;
  }
  if (nr & 1) return fail(KC_ERR_INVALID_ARG, "an interleaved file of %llu records: pairs need an even count", (unsigned long long)nr);
  *nreads = nr;
  *nbytes = nb;
  if (!fits && (nr || nb))
    return fail(KC_ERR_CAPACITY, "%llu reads with %llu bases do not fit the arrays", (unsigned long long)nr, (unsigned long long)nb);
  return KC_OK;
}

// ---- FASTQ front end on the device (kc_fastq.hpp) ------------------------------------------------------------------
// kc_fastq_to_packed_device (two = -1: one file, packed output) and kc_fastq_pairs_device (two = 0: one interleaved
// file, 1: two files).  The kernels find each file's first structural and first base error; fq_walk rebuilds the host
// parser's walk from them (fq_next's order, and the pairs' alternation), its status and its kc_last_error text.
struct FqJob {
  int two, nf;
  bool partial;
  FqFile f[2];
  uint64_t nout, nblk;  // output records in the sums' order, and their workgroups
  uint64_t *bsum;       // [nblk] per-workgroup sequence sums, then output offsets
  uint64_t h_ctl[2][FQC_N];
};

static dim3 fq_grid(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n, FQ_MAX_GRID))); }

// host text goes to context scratch in one copy per file; f[i].text, len and head are set either way
static int fq_stage_text(kc_ctx *c, FqJob &j, const char *const text_in[2], const uint64_t len_in[2], int on_device) {
  memset(j.f, 0, sizeof(j.f));
  for (int i = 0; i < j.nf; i++) {
    j.f[i].text = (const uint8_t *)text_in[i];
    j.f[i].len = len_in[i];
  }
  if (!on_device) {
    uint8_t *dst[2];
    auto layout = [&](uint8_t *base) {
      Carver m{base, 0};
      for (int i = 0; i < 2; i++) dst[i] = m.take<uint8_t>(j.f[i].len);
      return m.used + 256;
    };
    KCTRY(c->fq_text.reserve(layout(nullptr)));
    layout(c->fq_text.p);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < j.nf; i++) {
      if (j.f[i].len) HIPCHK(hipMemcpyAsync(dst[i], j.f[i].text, j.f[i].len, hipMemcpyHostToDevice, c->stream));
      j.f[i].text = dst[i];
    }
  }
  for (int i = 0; i < j.nf; i++) j.f[i].head = j.f[i].len ? (uint64_t)((uintptr_t)j.f[i].text & 15u) : 0;
  return KC_OK;
}

// count the lines, index them, check the records, sum the sequence lengths: leaves the control words of both files in
// j.h_ctl and the scanned sums in j.bsum, the stream idle
static int fq_index_lines(kc_ctx *c, FqJob &j) {
  FqFile *f = j.f;
  const int nf = j.nf;
  uint64_t ntiles_all = 0;
  for (int i = 0; i < nf; i++) {
    f[i].ntiles = (f[i].head + f[i].len + FQ_TILE - 1) / FQ_TILE;
    ntiles_all += f[i].ntiles;
  }
  uint64_t *d_ctl = nullptr;
  auto tiles = [&](uint8_t *base) {
    Carver m{base, 0};
    d_ctl = m.take<uint64_t>(2 * FQC_N);  // both files' control words, read back as one block (256 bytes: no padding)
    uint64_t *t = m.take<uint64_t>(ntiles_all);
    for (int i = 0; i < nf; i++) f[i].tile = t + (i ? f[0].ntiles : 0);
    return m.used;
  };
  KCTRY(c->fq_tiles.reserve(tiles(nullptr)));
  tiles(c->fq_tiles.p);
  for (int i = 0; i < 2; i++) f[i].ctl = d_ctl + i * FQC_N;  // (the second is unused with one file, read back all the same)
  HIPCHK(hipMemsetAsync(d_ctl, 0xFF, 2 * FQC_N * 8, c->stream));
  uint8_t last[2] = {'\n', '\n'};
  for (int i = 0; i < nf; i++) {
    if (f[i].ntiles) KCTRY(launch_timed(c, KT_FQ_COUNT, kc_fq_count_kernel, fq_grid(f[i].ntiles), dim3(FQ_TPB), 0, f[i]));
    KCTRY(launch_timed(c, KT_FQ_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{f[i].tile}}, f[i].ntiles,
                       f[i].ctl + FQC_NNL));
    if (f[i].len) HIPCHK(hipMemcpyAsync(&last[i], f[i].text + f[i].len - 1, 1, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(j.h_ctl, d_ctl, sizeof(j.h_ctl), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < nf; i++) {
    f[i].nnl = j.h_ctl[i][FQC_NNL];
    f[i].nl = f[i].nnl + (f[i].len && last[i] != '\n' ? 1 : 0);
  }
  if (j.partial) {  // whole records only: all four lines end in '\n' inside the text
    uint64_t w = f[0].nnl / 4;
    if (j.two == 0) w &= ~uint64_t(1);  // an interleaved file: whole pairs
    if (j.two > 0) w = std::min(w, f[1].nnl / 4);
    for (int i = 0; i < nf; i++) f[i].nl = 4 * w;
  }
  for (int i = 0; i < nf; i++) f[i].nrec = (f[i].nl + 3) / 4;
  j.nout = j.two > 0 ? 2 * std::max(f[0].nrec, f[1].nrec) : f[0].nrec;
  j.nblk = (j.nout + FQ_TPB - 1) / FQ_TPB;
  auto recs = [&](uint8_t *base) {
    Carver m{base, 0};
    for (int i = 0; i < nf; i++) {
      f[i].ends = m.take<uint64_t>(f[i].nnl);
      f[i].slen = m.take<uint64_t>(f[i].nrec);
    }
    j.bsum = m.take<uint64_t>(j.nblk);
    return m.used + 256;
  };
  KCTRY(c->fq_recs.reserve(recs(nullptr)));
  recs(c->fq_recs.p);
  if (nf == 1) f[1] = f[0];  // the kernels' second file is never read
  f[1].ctl = d_ctl + FQC_N;
  for (int i = 0; i < nf; i++) {
    if (f[i].ntiles && f[i].nnl) KCTRY(launch_timed(c, KT_FQ_INDEX, kc_fq_index_kernel, fq_grid(f[i].ntiles), dim3(FQ_TPB), 0, f[i]));
    if (f[i].nrec)
      KCTRY(launch_timed(c, KT_FQ_CHECK, kc_fq_check_kernel, fq_grid((f[i].nrec + FQ_TPB - 1) / FQ_TPB), dim3(FQ_TPB), 0, f[i]));
    KCTRY(launch_timed(c, KT_FQ_DETAIL, kc_fq_detail_kernel, dim3(1), dim3(64), 0, f[i]));
  }
  if (j.nout)
    KCTRY(launch_timed(c, KT_FQ_SUMS, kc_fq_sums_kernel, fq_grid(j.nblk), dim3(FQ_TPB), 0, f[0], f[1], j.two > 0 ? 1 : 0, j.nout, j.bsum));
  KCTRY(launch_timed(c, KT_FQ_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{j.bsum}}, j.nblk, f[0].ctl + FQC_TOTAL));
  HIPCHK(hipMemcpyAsync(j.h_ctl, d_ctl, sizeof(j.h_ctl), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

// The host parser's walk, from the control words the kernels left (no device call in here).  g: output records written
// before the walk stops; part_rec, part_len: the record a bad base cuts short in packed output (two < 0), else FQ_NONE.
// A status other than KC_OK comes with the host parser's text in kc_last_error.
struct FqWalk {
  int status;
  uint64_t g, part_rec, part_len;
};

static FqWalk fq_walk(const uint64_t h_ctl[2][FQC_N], const uint64_t nrec[2], int two) {
  const int nf = two > 0 ? 2 : 1;
  // Per file: t = the record where fq_next stops (its structural error, or the end after the sound records), bb = its
  // first record with a bad base if that comes before t.
  uint64_t t[2] = {0, 0}, bb[2] = {FQ_NONE, FQ_NONE};
  bool serr[2] = {false, false};
  for (int i = 0; i < nf; i++) {
    const uint64_t *k = h_ctl[i];
    const uint64_t valid = nrec[i] - (nrec[i] && k[FQC_END] == 1 ? 1 : 0);
    serr[i] = k[FQC_STRUCT] != FQ_NONE;
    t[i] = serr[i] ? k[FQC_STRUCT] : valid;
    if (k[FQC_BASE] < t[i]) bb[i] = k[FQC_BASE];
  }
  enum { EV_BASE, EV_STRUCT, EV_END } ev = EV_END;
  int evf = 0;     // the file the walk stops in
  uint64_t g = 0;  // output records written before it stops
  if (two > 0) {
    // record j of file 1 is step 2j of the walk, of file 2 step 2j + 1
    uint64_t best = FQ_NONE;
    auto take = [&](uint64_t step, int e, int fi) {
      if (step < best) {
        best = step;
        ev = (decltype(ev))e;
        evf = fi;
      }
    };
    for (int i = 0; i < 2; i++) {
      if (bb[i] != FQ_NONE) take(2 * bb[i] + i, EV_BASE, i);
      take(2 * t[i] + i, serr[i] ? EV_STRUCT : EV_END, i);
    }
    g = best;
  } else {
    ev = bb[0] != FQ_NONE ? EV_BASE : serr[0] ? EV_STRUCT : EV_END;
    g = ev == EV_BASE ? bb[0] : t[0];
  }
  FqWalk w = {KC_OK, g, FQ_NONE, 0};
  const uint64_t *k = h_ctl[evf];
  const uint64_t r = two > 0 ? g >> 1 : g;  // the record of file evf
  if (ev == EV_BASE) {
    if (two < 0) {
      w.status = fail(KC_ERR_BAD_BASE, "Illegal char in comp nucleotide (int=%d) at line %llu", (int)k[FQC_BYTE], (unsigned long long)(4 * r + 2));
      w.part_rec = g;
      w.part_len = k[FQC_POS];
    } else {
      w.status = fail(KC_ERR_BAD_BASE, "Illegal char in comp nucleotide (int=%d) at line %llu of file %d", (int)k[FQC_BYTE],
                      (unsigned long long)(4 * r + 2), evf + 1);
    }
  } else if (ev == EV_END && two > 0 && evf == 1) {
    w.status = fail(KC_ERR_INVALID_ARG, "the second file ends after %llu records, the first has more", (unsigned long long)t[1]);
  } else if (ev == EV_END && two > 0 && t[1] > t[0]) {  // file 1 ended; file 2's next record is sound
    w.status = fail(KC_ERR_INVALID_ARG, "the first file ends after %llu records, the second has more", (unsigned long long)t[0]);
  } else if (ev == EV_STRUCT || (ev == EV_END && two > 0 && serr[1] && t[1] == t[0])) {
    int fi = ev == EV_STRUCT ? evf : 1;  // (or file 2's record after file 1's end is malformed)
    const uint64_t *kk = h_ctl[fi];
    const unsigned long long rr = (unsigned long long)t[fi];
    const int e = KC_ERR_INVALID_ARG;
    switch ((int)kk[FQC_KIND]) {
      case FQK_TRUNCATED: w.status = fail(e, "FASTQ ends inside the record that starts at line %llu", 4 * rr + 1); break;
      case FQK_NAME: w.status = fail(e, "Invalid FASTQ: expected read name (@) at line %llu", 4 * rr + 1); break;
      case FQK_PLUS: w.status = fail(e, "Invalid FASTQ: expected '+' at line %llu", 4 * rr + 3); break;
      default:
        w.status = fail(e, "Invalid FASTQ: sequence length %llu != %llu quals length at line %llu", (unsigned long long)kk[FQC_A],
                        (unsigned long long)kk[FQC_B], 4 * rr + 2);
    }
  } else if (two == 0 && (g & 1)) {
    w.status = fail(KC_ERR_INVALID_ARG, "an interleaved file of %llu records: pairs need an even count", (unsigned long long)g);
  }
  return w;
}

// the records the host parser would have written before it stopped, then its status or the capacity verdict
static int fq_write(kc_ctx *c, const FqJob &j, const FqWalk &w, uint8_t *d_packed, uint8_t *d_bases, uint8_t *d_quals, uint64_t capacity,
                    uint64_t *d_offsets, uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes) {
  const bool packed = j.two < 0;
  const uint64_t nr = w.g, nb = j.h_ctl[0][FQC_TOTAL];
  const bool arrays = d_offsets && (packed ? d_packed != nullptr : (d_bases && d_quals));
  if (d_offsets && reads_capacity + 1 > 0) HIPCHK(hipMemsetAsync(d_offsets, 0, 8, c->stream));
  if (arrays && (w.g || w.part_rec != FQ_NONE) && w.g <= j.nout && (w.part_rec == FQ_NONE || w.part_rec < j.nout)) {  // (always, by construction)
    FqOut o;
    memset(&o, 0, sizeof(o));
    o.packed = d_packed;
    o.bases = d_bases;
    o.quals = d_quals;
    o.offsets = d_offsets;
    o.cap = capacity;
    o.reads_cap = reads_capacity;
    o.nout = j.nout;
    o.lim = w.g;
    o.part_rec = w.part_rec;
    o.part_len = w.part_len;
    o.bsum = j.bsum;
    o.qoff = c->cfg.qual_offset;
    const dim3 grid = fq_grid(((w.part_rec != FQ_NONE ? w.part_rec + 1 : w.g) + FQ_TPB - 1) / FQ_TPB);
    if (packed)
      KCTRY(launch_timed(c, KT_FQ_WRITE_PACKED, kc_fq_write_kernel<true>, grid, dim3(FQ_TPB), 0, j.f[0], j.f[1], 0, o));
    else
      KCTRY(launch_timed(c, KT_FQ_WRITE_PAIRS, kc_fq_write_kernel<false>, grid, dim3(FQ_TPB), 0, j.f[0], j.f[1], j.two > 0 ? 1 : 0, o));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (w.status) return w.status;
  *nreads = nr;
  *nbytes = nb;
  const bool fits = arrays && nr <= reads_capacity && nb <= capacity;
  if (!fits && (nr || nb))
    return fail(KC_ERR_CAPACITY, "%llu reads with %llu bases do not fit the arrays", (unsigned long long)nr, (unsigned long long)nb);
  return KC_OK;
}

static int fq_device(kc_ctx *c, const char *const text_in[2], const uint64_t len_in[2], int two, int on_device, uint32_t flags,
                     uint8_t *d_packed, uint8_t *d_bases, uint8_t *d_quals, uint64_t capacity, uint64_t *d_offsets,
                     uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes, uint64_t *consumed[2]) {
  FqJob j;
  j.two = two;
  j.nf = two > 0 ? 2 : 1;
  if (!c || !nreads || !nbytes || (flags & ~KC_FASTQ_PARTIAL)) return KC_ERR_INVALID_ARG;
  for (int i = 0; i < j.nf; i++)
    if (len_in[i] && !text_in[i]) return KC_ERR_INVALID_ARG;
  j.partial = (flags & KC_FASTQ_PARTIAL) != 0;
  HIPCHK(hipSetDevice(c->cfg.device));
  KCTRY(fq_stage_text(c, j, text_in, len_in, on_device));
  KCTRY(fq_index_lines(c, j));
  for (int i = 0; i < j.nf; i++)
    if (consumed[i]) *consumed[i] = j.partial ? j.h_ctl[i][FQC_CONSUMED] : len_in[i];
  const uint64_t nrec[2] = {j.f[0].nrec, j.f[1].nrec};
  const FqWalk w = fq_walk(j.h_ctl, nrec, two);
  return fq_write(c, j, w, d_packed, d_bases, d_quals, capacity, d_offsets, reads_capacity, nreads, nbytes);
}

extern "C" int kc_fastq_to_packed_device(kc_ctx *c, const char *text, uint64_t len, int on_device, uint32_t flags, uint8_t *d_packed,
                                         uint64_t packed_capacity, uint64_t *d_offsets, uint64_t reads_capacity, uint64_t *nreads,
                                         uint64_t *nbytes, uint64_t *consumed) {
  const char *t[2] = {text, nullptr};
  const uint64_t l[2] = {len, 0};
  uint64_t *cons[2] = {consumed, nullptr};
  return fq_device(c, t, l, -1, on_device, flags, d_packed, nullptr, nullptr, packed_capacity, d_offsets, reads_capacity, nreads, nbytes,
                   cons);
}

extern "C" int kc_fastq_pairs_device(kc_ctx *c, const char *text1, uint64_t len1, const char *text2, uint64_t len2, int on_device,
                                     uint32_t flags, uint8_t *d_bases, uint8_t *d_quals, uint64_t capacity, uint64_t *d_offsets,
                                     uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes, uint64_t *consumed1,
                                     uint64_t *consumed2) {
  const char *t[2] = {text1, text2};
  const uint64_t l[2] = {len1, len2};
  uint64_t *cons[2] = {consumed1, consumed2};
  return fq_device(c, t, l, text2 ? 1 : 0, on_device, flags, nullptr, d_bases, d_quals, capacity, d_offsets, reads_capacity, nreads,
                   nbytes, cons);
}

// ---- overlap merge of read pairs (kc_merge.hpp) --------------------------------------------------------------------
extern "C" int kc_merge_pairs(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t npairs,
                              int on_device, int min_kmer_len, uint8_t *d_packed, uint64_t packed_capacity, uint64_t *d_out_offsets,
                              uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes, kc_merge_stats *stats) {
  if (!c || !nreads || !nbytes || min_kmer_len < 0 || (npairs && (!bases || !quals || !offsets))) return KC_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->cfg.device));
  kc_merge_stats ms;
  memset(&ms, 0, sizeof(ms));
  ms.pairs = npairs;
  *nreads = *nbytes = 0;
  if (stats) *stats = ms;
  if (d_out_offsets && reads_capacity + 1 > 0) HIPCHK(hipMemsetAsync(d_out_offsets, 0, 8, c->stream));
  if (!npairs) {
    HIPCHK(hipStreamSynchronize(c->stream));
    return KC_OK;
  }
  if (npairs > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;  // pair indices of the long-pair list are 32-bit
  if (!on_device) KCTRY(stage_host_reads(c, &bases, &quals, &offsets, 2 * npairs));
  const uint64_t ntiles = (npairs + MG_TILE - 1) / MG_TILE;
  MergeArgs a;
  memset(&a, 0, sizeof(a));
  a.bases = bases;
  a.quals = quals;
  a.offsets = offsets;
  a.npairs = npairs;
  a.qoff = c->cfg.qual_offset;
  a.min_len = min_kmer_len ? min_kmer_len : c->k;
  size_t zeroed = 0;
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    a.pair_dec = m.take<uint32_t>(npairs);
    a.pair_out = m.take<uint32_t>(npairs);
    a.long_list = m.take<uint32_t>(npairs);
    a.tile_bytes = m.take<uint64_t>(ntiles);
    a.tile_reads = m.take<uint64_t>(ntiles);
    zeroed = m.used;  // from here to the end, one memset: the statistics and the control block stay the layout's tail
    a.stats = m.take<uint64_t>(MG_SLOTS * MGS_N);
    a.ctl = m.take<uint32_t>(64);  // [MG_CTL_N], the totals at word 16
    a.totals = (uint64_t *)(a.ctl + 16);
    return m.used;
  };
  const size_t need = layout(nullptr);
  KCTRY(c->mg.reserve(need));
  layout(c->mg.p);
  a.out = d_packed;
  a.out_offsets = d_out_offsets;
  HIPCHK(hipMemsetAsync(a.stats, 0, need - zeroed, c->stream));
  KCTRY(launch_timed(c, KT_MERGE_DECIDE, kc_merge_decide_kernel, dim3((unsigned)ntiles), dim3(64 * MG_WAVES), 0, a));
  uint32_t ctl[MG_CTL_N];
  HIPCHK(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint32_t nlong = ctl[MG_CTL_NLONG];
  const int lcap = (int)((ctl[MG_CTL_LONGMAX] + 3) & ~3u);
  const size_t lbytes = 4 * ((size_t)lcap + MG_PAD);
  if (nlong && !ctl[MG_CTL_ERR]) {
    KCTRY(set_dyn_lds(kc_merge_decide_long_kernel, lbytes));
    KCTRY(set_dyn_lds(kc_merge_write_long_kernel, lbytes));
    KCTRY(launch_timed(c, KT_MERGE_DECIDE_LONG, kc_merge_decide_long_kernel, dim3(nlong), dim3(64), lbytes, a, lcap));
    HIPCHK(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (ctl[MG_CTL_ERR] & MG_ERR_BASE) return fail(KC_ERR_BAD_BASE, "kc_merge_pairs: a read holds a byte outside ACGTN/acgtn/IUPAC");
  if (ctl[MG_CTL_ERR])
    return fail(KC_ERR_INVALID_ARG, "kc_merge_pairs: a quality outside [qual_offset, qual_offset + 80] or a mate longer than %d", MG_MAX_LEN);
  KCTRY(launch_timed(c, KT_MERGE_SCAN, kc_scan_kernel<2>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<2>{{a.tile_bytes, a.tile_reads}}, ntiles,
                     a.totals));
  uint64_t tot[2], hs[MG_SLOTS * MGS_N];
  HIPCHK(hipMemcpyAsync(tot, a.totals, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hs, a.stats, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int s = 0; s < MG_SLOTS; s++) {
    ms.merged += hs[s * MGS_N + MGS_MERGED];
    ms.ambiguous += hs[s * MGS_N + MGS_AMBIG];
    ms.dropped += hs[s * MGS_N + MGS_DROPPED];
    ms.overlap_len += hs[s * MGS_N + MGS_OVERLAP];
    ms.merged_len += hs[s * MGS_N + MGS_MERGED_LEN];
  }
  ms.out_bases = tot[0];
  ms.out_reads = tot[1];
  *nbytes = tot[0];
  *nreads = tot[1];
  if (stats) *stats = ms;
  if (!d_packed || !d_out_offsets || tot[0] > packed_capacity || tot[1] > reads_capacity) {
    if (!tot[0] && !tot[1]) return KC_OK;
    return fail(KC_ERR_CAPACITY, "%llu merged reads with %llu bases do not fit the arrays", (unsigned long long)tot[1], (unsigned long long)tot[0]);
  }
  KCTRY(launch_timed(c, KT_MERGE_WRITE, kc_merge_write_kernel, dim3((unsigned)ntiles), dim3(64 * MG_WAVES), 0, a));
  if (nlong) KCTRY(launch_timed(c, KT_MERGE_WRITE_LONG, kc_merge_write_long_kernel, dim3(nlong), dim3(64), lbytes, a, lcap));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}

// ---- adapter trimming (kc_trim.hpp) ---------------------------------------------------------------------------------
namespace {
struct HostAdapters {
  std::vector<std::string> entries;  // s at 2n, revcomp(s) at 2n+1
  uint64_t n_short = 0;
  std::vector<uint64_t> keys;                 // distinct k-mers in order of first insertion
  std::vector<std::vector<uint32_t>> records; // per k-mer: entry << TR_REC_OFF_BITS | offset, in insertion order
};
}  // namespace

// revcomp, src/utils.cpp:98-129; false for a byte the reference DIEs on
static bool adapters_revcomp(const std::string &s, std::string &rc) {
  rc.clear();
  rc.reserve(s.size());
  for (size_t i = s.size(); i-- > 0;) {
    switch (s[i]) {
      case 'A': case 'a': rc += 'T'; break;
      case 'C': case 'c': rc += 'G'; break;
      case 'G': case 'g': rc += 'C'; break;
      case 'T': case 't': rc += 'A'; break;
      case 'N': case 'n':
      case 'U': case 'R': case 'Y': case 'K': case 'M': case 'S': case 'W': case 'B': case 'D': case 'H': case 'V': rc += 'N'; break;
      default: return false;
    }
  }
  return true;
}

// Adapters::load_adapter_seqs (src/adapters.cpp:48-146) on a text in memory
static int adapters_build(const char *text, uint64_t len, int k, HostAdapters &h) {
  if (k < 1 || (len && !text)) return KC_ERR_INVALID_ARG;
  if (k > TR_MAX_K) return fail(KC_ERR_UNSUPPORTED_K, "adapter_k %d is above MAX_ADAPTER_K = %d", k, TR_MAX_K);
  uint64_t lineno = 0;
  for (uint64_t p = 0; p < len;) {  // getline: a last line without '\n' counts, nothing after the last '\n' does not
    const char *nl = (const char *)memchr(text + p, '\n', len - p);
    const uint64_t e = nl ? (uint64_t)(nl - text) : len;
    const uint64_t n = e - p;
    lineno++;
    if (!(n && text[p] == '>')) {
      if (n < (uint64_t)k) {
        h.n_short++;
      } else {
        if (n > (uint64_t)TR_MAX_ENTRY_LEN)
          return fail(KC_ERR_INVALID_ARG, "adapter of %llu bases in line %llu: at most %d", (unsigned long long)n, (unsigned long long)lineno,
                      TR_MAX_ENTRY_LEN);
        if (h.entries.size() + 2 > (size_t)TR_MAX_ENTRIES) return fail(KC_ERR_INVALID_ARG, "more than %d adapter sequences", TR_MAX_ENTRIES / 2);
        std::string s(text + p, (size_t)n), rc;
        if (!adapters_revcomp(s, rc))
          return fail(KC_ERR_BAD_BASE, "adapter in line %llu holds a byte revcomp does not take", (unsigned long long)lineno);
        h.entries.push_back(std::move(s));
        h.entries.push_back(std::move(rc));
      }
    }
    p = e + 1;
  }
  std::unordered_map<uint64_t, uint32_t> ids;
  const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull;
  for (size_t e = 0; e < h.entries.size(); e++) {
    const std::string &s = h.entries[e];
    uint64_t key = 0;
    for (size_t j = 0; j < s.size(); j++) {  // base p of a k-mer in bits 2p, 2p+1 (tr_seed_keys)
      key = (key >> 2) | ((uint64_t)tr_kcode((uint8_t)s[j]) << (2 * (k - 1)));
      if (j + 1 < (size_t)k) continue;
      const uint64_t kk = key & mask;
      auto it = ids.find(kk);
      uint32_t id;
      if (it == ids.end()) {
        id = (uint32_t)h.keys.size();
        ids.emplace(kk, id);
        h.keys.push_back(kk);
        h.records.emplace_back();
      } else {
        id = it->second;
      }
      h.records[id].push_back((uint32_t)(e << TR_REC_OFF_BITS) | (uint32_t)(j + 1 - k));
    }
  }
  return KC_OK;
}

static void adapters_counts(const HostAdapters &h, uint64_t *n_adapters, uint64_t *n_short, uint64_t *n_entries, uint64_t *n_kmers) {
  if (n_adapters) *n_adapters = h.entries.size() / 2;
  if (n_short) *n_short = h.n_short;
  if (n_entries) *n_entries = h.entries.size();
  if (n_kmers) *n_kmers = h.keys.size();
}

extern "C" int kc_adapters_index(const char *text, uint64_t len, int adapter_k, uint64_t *n_adapters, uint64_t *n_short,
                                 uint64_t *n_entries, uint64_t *n_kmers) {
  HostAdapters h;
  const int rc = adapters_build(text, len, adapter_k, h);
  if (rc) return rc;
  adapters_counts(h, n_adapters, n_short, n_entries, n_kmers);
  return KC_OK;
}

extern "C" int kc_adapters_clear(kc_ctx *c) {
  if (!c) return KC_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(c->d_ad.release());
  c->ad_recs = c->ad_ent_off = nullptr;
  c->ad_bytes = nullptr;
  c->ad_loaded = false;
  c->ad_entries = 0;
  return KC_OK;
}

extern "C" int kc_adapters_load(kc_ctx *c, const char *text, uint64_t len, int adapter_k, uint32_t flags, uint64_t *n_adapters,
                                uint64_t *n_short, uint64_t *n_entries, uint64_t *n_kmers) {
  if (!c || adapter_k < 0 || (flags & ~KC_ADAPTERS_BLASTN_SCORES)) return KC_ERR_INVALID_ARG;
  const int k = adapter_k ? adapter_k : c->k;
  HostAdapters h;
  KCTRY(adapters_build(text, len, k, h));
  // the device image: the k-mer table at most half full, the records, the entries' offsets and bytes
  uint32_t lg = 4;
  while ((1ull << lg) < 2 * h.keys.size()) lg++;
  std::vector<TrSlot> slots((size_t)1 << lg);
  memset(slots.data(), 0, slots.size() * sizeof(TrSlot));
  std::vector<uint32_t> recs;
  for (size_t i = 0; i < h.keys.size(); i++) {
    uint32_t s = tr_hash(h.keys[i], lg);
    while (slots[s].rec_count) s = (s + 1) & ((1u << lg) - 1u);
    slots[s].key = h.keys[i];
    slots[s].rec_start = (uint32_t)recs.size();
    slots[s].rec_count = (uint32_t)h.records[i].size();
    recs.insert(recs.end(), h.records[i].begin(), h.records[i].end());
  }
  std::vector<uint32_t> ent_off(h.entries.size() + 1, 0);
  std::string bytes;
  for (size_t e = 0; e < h.entries.size(); e++) {
    ent_off[e] = (uint32_t)bytes.size();
    bytes += h.entries[e];
  }
  ent_off[h.entries.size()] = (uint32_t)bytes.size();
  TrSlot *d_slots = nullptr;
  uint32_t *d_recs = nullptr, *d_ent = nullptr;
  uint8_t *d_bytes = nullptr;
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    d_slots = m.take<TrSlot>(slots.size());
    d_recs = m.take<uint32_t>(recs.size() + 1);
    d_ent = m.take<uint32_t>(ent_off.size());
    d_bytes = m.take<uint8_t>(bytes.size() + 1);
    return m.used;
  };
  KCTRY(kc_adapters_clear(c));  // loading again replaces the set
  KCTRY(c->d_ad.reserve(layout(nullptr)));
  layout(c->d_ad.p);
  HIPCHK(hipMemcpy(d_slots, slots.data(), slots.size() * sizeof(TrSlot), hipMemcpyHostToDevice));
  if (!recs.empty()) HIPCHK(hipMemcpy(d_recs, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_ent, ent_off.data(), ent_off.size() * 4, hipMemcpyHostToDevice));
  if (!bytes.empty()) HIPCHK(hipMemcpy(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  c->ad_recs = d_recs;
  c->ad_ent_off = d_ent;
  c->ad_bytes = d_bytes;
  c->ad_lg_slots = lg;
  c->ad_entries = (uint32_t)h.entries.size();
  c->ad_k = k;
  c->ad_blastn = (flags & KC_ADAPTERS_BLASTN_SCORES) ? 1 : 0;
  c->ad_loaded = true;
  adapters_counts(h, n_adapters, n_short, n_entries, n_kmers);
  return KC_OK;
}

extern "C" int kc_trim_adapters(kc_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                                int on_device, uint32_t flags, uint8_t *d_out_bases, uint8_t *d_out_quals, uint64_t capacity,
                                uint64_t *d_out_offsets, uint64_t *nbytes, kc_trim_stats *stats) {
  if (!c || !nbytes || (flags & ~KC_TRIM_PAIRED) || (nreads && (!bases || !quals || !offsets))) return KC_ERR_INVALID_ARG;
  const int paired = (flags & KC_TRIM_PAIRED) ? 1 : 0;
  if (paired && (nreads & 1)) return fail(KC_ERR_INVALID_ARG, "kc_trim_adapters: KC_TRIM_PAIRED with an odd number of reads");
  if (!c->ad_loaded) return fail(KC_ERR_STATE, "kc_trim_adapters: no adapter set is loaded (kc_adapters_load)");
  HIPCHK(hipSetDevice(c->cfg.device));
  kc_trim_stats ts;
  memset(&ts, 0, sizeof(ts));
  ts.reads = nreads;
  *nbytes = 0;
  if (stats) *stats = ts;
  if (d_out_offsets) HIPCHK(hipMemsetAsync(d_out_offsets, 0, 8, c->stream));
  if (!nreads) {
    HIPCHK(hipStreamSynchronize(c->stream));
    return KC_OK;
  }
  if (nreads > 0xFFFFFFFFull) return KC_ERR_INVALID_ARG;  // read indices of the hit list are 32-bit
  if (!on_device) KCTRY(stage_host_reads(c, &bases, &quals, &offsets, nreads));
  const uint64_t ntiles = (nreads + TR_TILE - 1) / TR_TILE;
  TrimArgs a;
  memset(&a, 0, sizeof(a));
  a.bases = bases;
  a.quals = quals;
  a.offsets = offsets;
  a.nreads = nreads;
  a.k = c->ad_k;
  a.paired = paired;
  a.match = c->ad_blastn ? 2 : 1;  // BLASTN_ALN_SCORES 23521 / ALTERNATE_ALN_SCORES 11111
  a.mismatch = c->ad_blastn ? 3 : 1;
  a.gap_open = c->ad_blastn ? 5 : 1;
  a.gap_ext = c->ad_blastn ? 2 : 1;
  a.amb = 1;
  a.slots = c->d_ad.as<const TrSlot>();
  a.lg_slots = c->ad_lg_slots;
  a.slot_mask = (1u << c->ad_lg_slots) - 1u;
  a.recs = c->ad_recs;
  a.ent_off = c->ad_ent_off;
  a.ent_bytes = c->ad_bytes;
  a.n_entries = c->ad_entries;
  auto layout = [&](uint8_t *base) {
    Carver m{base, 0};
    a.res = m.take<uint32_t>(nreads);
    a.flen = m.take<uint32_t>(nreads);
    a.list = m.take<uint32_t>(nreads);
    a.tile_bytes = m.take<uint64_t>(ntiles);
    a.ctl = m.take<uint32_t>(64);  // zeroed: [TR_CTL_N], the statistics at word 8, the scan's total at word 24
    return m.used;
  };
  KCTRY(c->tr.reserve(layout(nullptr)));
  layout(c->tr.p);
  a.stats = (unsigned long long *)(a.ctl + 8);
  uint64_t *total = (uint64_t *)(a.ctl + 24);
  a.out_bases = d_out_bases;
  a.out_quals = d_out_quals;
  a.out_offsets = d_out_offsets;
  HIPCHK(hipMemsetAsync(a.ctl, 0, 64 * 4, c->stream));
  const uint64_t per = (uint64_t)TR_SEED_WAVES * TR_RPW;
  KCTRY(launch_timed(c, KT_TRIM_SEED, kc_trim_seed_kernel, dim3((unsigned)((nreads + per - 1) / per)), dim3(64 * TR_SEED_WAVES), 0, a));
  uint32_t ctl[TR_CTL_N];
  HIPCHK(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (ctl[TR_CTL_ERR]) return fail(KC_ERR_INVALID_ARG, "kc_trim_adapters: a read longer than %d, or offsets that decrease", MG_MAX_LEN);
  if (const uint32_t nlist = ctl[TR_CTL_NLIST]) {
    const unsigned grid = (unsigned)std::min<uint64_t>(nlist, (uint64_t)c->num_cus * 32);
    KCTRY(launch_timed(c, KT_TRIM_ALIGN, kc_trim_align_kernel, dim3(grid), dim3(64), 0, a, nlist));
  }
  KCTRY(launch_timed(c, KT_TRIM_SIZES, kc_trim_sizes_kernel, dim3((unsigned)ntiles), dim3(TR_TILE), 0, a));
  KCTRY(launch_timed(c, KT_TRIM_SCAN, kc_scan_kernel<1>, dim3(1), dim3(SCAN_TPB), 0, ScanArrays<1>{{a.tile_bytes}}, ntiles, total));
  uint64_t tot[1];
  unsigned long long hs[TRS_N];
  HIPCHK(hipMemcpyAsync(tot, total, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hs, a.stats, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  ts.trimmed = hs[TRS_TRIMMED];
  ts.bases_trimmed = hs[TRS_BASES];
  ts.reads_removed = hs[TRS_REMOVED];
  ts.alignments = hs[TRS_ALIGN];
  ts.out_bases = tot[0];
  *nbytes = tot[0];
  if (stats) *stats = ts;
  if (!d_out_bases || !d_out_quals || !d_out_offsets || tot[0] > capacity)
    return fail(KC_ERR_CAPACITY, "%llu trimmed reads with %llu bases do not fit the arrays", (unsigned long long)nreads, (unsigned long long)tot[0]);
  KCTRY(launch_timed(c, KT_TRIM_WRITE, kc_trim_write_kernel, dim3((unsigned)ntiles), dim3(TR_TILE), 0, a));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KC_OK;
}
