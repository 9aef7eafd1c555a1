/* kcount_mi355_polish.h -- the third public header of libkcount_mi355.so: contigs polished from the pileup of the reads'
 * gapped records (tests/polish_model.py).  It includes kcount_mi355.h and adds one entry point.  The
 * entry point has a header of its own because tests/test_abi.py and tests/test_entry_point_coverage_all.py hold the first
 * header to closed lists; tests/test_entry_point_coverage_polish.py holds this one to the same rule.
 */
#ifndef KCOUNT_MI355_POLISH_H
#define KCOUNT_MI355_POLISH_H

#include "kcount_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kc_ctg_polish: every column of the indexed block rewritten to the clear winner of its pileup -------------------------
 * The reference holds no contig or alignment code, so the rules are this project's own.  Substitutions only: no length
 * changes, so offsets, depths, links and scaffold member records stay valid over the polished block.
 *
 * Input: the kept contig index (kc_ctg_index_build), whose block of nbytes bytes and n_ctgs contigs kc_ctg_index_info
 * reports; the reads (bases, offsets, nreads, as kc_align_gapped takes them; quals may be NULL and has the bases' bytes
 * beside them) and n_alns records of kc_align_gapped.
 *
 * Codes are kc_align_gapped's: a read's A C G T in either case are 0 .. 3, any other byte 4; a contig's byte likewise (its N
 * is 4).  R' is the read for orient 0 and its reverse complement for orient 1; with L the read's length the quality of R'[r]
 * is quals[r] for orient 0 and quals[L - 1 - r] for orient 1, less the context's qual_offset.
 *
 * A record is valid, and passes the filter (min_score, min_len), by kc_aln_depths' definitions; read < nreads and
 * rstop <= L(read) always belong to validity here.  With KC_POLISH_BEST_ONLY only a read's best record (kc_aln_depths'
 * definition) takes part.  With span = cstop - cstart every record falls in exactly one class, the first that applies:
 *   none       kind is KC_GAP_NONE
 *   filtered   it does not pass the filter
 *   not_best   KC_POLISH_BEST_ONLY and it is not its read's best record
 *   unequal    span != rstop - rstart: not one diagonal
 *   divergent  m > max_mismatches, m the number of i in [0, span) at which R'[rstart + i] and contig[cstart + i] both have
 *              a code < 4 and differ (the record's own mismatches field is not read)
 *   placed     every other record.
 * A placed record votes at i in [e_lo, span - e_hi), e_lo = cstart > 0 ? edge_clip : 0, e_hi = cstop < len_u ? edge_clip : 0:
 * with b the code of R'[rstart + i] it adds 1 to cnt[cstart + i][b] iff b < 4 and quals is NULL, or min_qual is 0, or the
 * quality is >= min_qual.
 *
 * A column has the counts c0 .. c3 (exact in 32 bits), tot their sum, top the largest, w the lowest code that holds it,
 * second the largest of the other three, cur the contig byte's code.  Its class is the first that applies:
 *   uncovered  tot == 0
 *   thin       tot < min_depth
 *   disputed   top == second, or top * 1000 < min_permille * tot (in 64 bits)
 *   confirmed  w == cur
 *   changed    the byte becomes "ACGT"[w]; it is also `filled` when cur is 4.
 * Every byte that is not changed is copied, separators too.
 *
 * out (nbytes bytes) is the block again.  counts (may be NULL): nbytes * 4 values min(c, 65535), a column's four side by
 * side, 0 on separators.  ctgs (may be NULL): a record per contig.  fixes (may be NULL): a record per changed column in
 * ascending position; more than fix_capacity of them is KC_ERR_CAPACITY, never a truncation; fixes == NULL needs no capacity.
 * Every output is one exact byte string that does not depend on the order of the records.
 *
 * KC_ERR_INVALID_ARG before the context, with no device: params NULL, edge_clip over KC_DEPTH_MAX_EDGE, min_depth 0,
 * min_permille over 1000, min_qual over 255, unknown flags; then NULL ctx / out / offsets with reads / alns with records,
 * misaligned device arrays (records 16 bytes, offsets 8, counts 2).  KC_ERR_STATE without an index.  KC_ERR_CAPACITY for 2^32
 * records or reads or more.  From the device checks, before anything is stored: KC_ERR_INVALID_ARG for a read over
 * KC_ALIGN_MAX_READ_LEN or decreasing offsets, and for an invalid record, the lowest bad index named.  On every error nothing
 * is written through any pointer.  n_alns == 0 is KC_OK with out equal to the block.  The index, the table and the results
 * are untouched; the call runs on the context's stream, works with rank_n > 1, and its scratch (24 bytes a record and the
 * copies of host arrays) lives for the call.  on_device != 0: every array but params and stats is a device pointer.
 */
#define KC_POLISH_BEST_ONLY 1u
typedef struct kc_polish_params { /* 32 bytes */
  uint32_t min_score, min_len;     /* the filter, as kc_aln_depths' */
  uint32_t edge_clip;              /* at most KC_DEPTH_MAX_EDGE */
  uint32_t max_mismatches;         /* a record with more is divergent */
  uint32_t min_depth;              /* at least 1 */
  uint32_t min_permille;           /* at most 1000: the winner's share of the votes */
  uint32_t min_qual;               /* 0: no gate; at most 255 */
  uint32_t flags;                  /* KC_POLISH_BEST_ONLY */
} kc_polish_params;
typedef struct kc_polish_ctg { /* 32 bytes, one per contig */
  uint64_t votes;               /* the sum of tot over the contig's columns */
  uint32_t placed;              /* placed records */
  uint32_t changed, filled, disputed, thin, uncovered; /* columns */
} kc_polish_ctg;
typedef struct kc_polish_fix { /* 16 bytes */
  uint32_t pos;                 /* position in the block */
  uint32_t ctg;
  uint8_t old_base, new_base;   /* the bytes */
  uint16_t top, tot;            /* min(top, 65535), min(tot, 65535) */
  uint16_t pad;                 /* zero */
} kc_polish_fix;
typedef struct kc_polish_stats { /* 128 bytes */
  uint64_t records, none, filtered, not_best, unequal, divergent, placed;
  uint64_t votes;               /* the sum of tot over all columns */
  uint64_t columns;             /* nbytes - n_ctgs */
  uint64_t uncovered, thin, disputed, confirmed, changed, filled;
  uint64_t sort_passes;         /* radix passes of the sort by position */
} kc_polish_stats;
int kc_ctg_polish(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                  const kc_gap_aln *alns, uint64_t n_alns, int on_device, const kc_polish_params *params, uint8_t *out,
                  uint16_t *counts, kc_polish_ctg *ctgs, kc_polish_fix *fixes, uint64_t fix_capacity, kc_polish_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
