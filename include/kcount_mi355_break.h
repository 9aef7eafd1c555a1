/* kcount_mi355_break.h -- the fourth public header of libkcount_mi355.so: contigs cut where no read pair spans them and the
 * mates that should have spanned landed elsewhere (tests/break_model.py).  It includes kcount_mi355.h
 * and adds one entry point.  The entry point has a header of its own for the reason the second and third have: existing
 * tests hold the earlier headers and binding tables to closed lists; tests/test_entry_point_coverage_break.py holds this
 * one to the same rule.
 */
#ifndef KCOUNT_MI355_BREAK_H
#define KCOUNT_MI355_BREAK_H

#include "kcount_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kc_ctg_break: the indexed block with a separator put in wherever the pairs say a contig is a false join ------------------
 * The reference holds no contig code, so the rules are this project's own.  A check of physical (fragment) coverage: a
 * column is suspect when few proper pairs span it and many mates whose partner should lie across it have their partner
 * elsewhere.  No base is dropped or changed; a contig only falls into pieces.
 *
 * Input: the kept contig index (kc_ctg_index_build), whose block of nbytes bytes and n_ctgs contigs kc_ctg_index_info
 * reports; the reads' nreads + 1 offsets (no bases; nreads is even, reads 2p and 2p + 1 are mates); n_alns records of
 * kc_align_gapped in any order; nreads / 2 records of kc_pair_inserts; optionally depths, uint16_t[nbytes] in the layout of
 * kc_submit_ctg_block.  A record is valid by kc_aln_depths' definition, with read < nreads and rstop <= L(read); a pair
 * record is valid by kc_local_assm's rule (aln0 / aln1 are 0xFFFFFFFF or name a record of read 2p / 2p + 1 that is not
 * KC_GAP_NONE).  A pair record's cls and insert are NOT read: the call classifies the pair again from its two records, so
 * a forged class can never put an interval out of range.
 *
 * All arithmetic is integer, signed 64-bit where differences are taken.  L(.) is a read's length.
 *
 * Pairs.  Pair p has A0 = the record aln0 names and A1 = the record aln1 names; either may be absent.
 *   both present, same contig u, different orient: F the orient-0 record, R the orient-1 record, fs = F.cstart - F.rstart,
 *     rs = R.cstart - R.rstart, re = R.cstop + (L_R - R.rstop) (kc_pair_inserts' quantities).  If rs >= fs and
 *     re - fs <= max_insert the pair is SPANNING and adds 1 to span[j] for j in [max(fs, 0), min(re, len_u)) of contig u, iff
 *     that interval is not empty.  Otherwise both mates are DISCORDANT.
 *   both present, on different contigs or with equal orient: both mates are discordant (a DISCORDANT PAIR either way).
 *   exactly one present (ONE MATE): that mate is discordant iff KC_BREAK_ONE_MATE, otherwise ignored.
 *   neither present: NONE.
 * A discordant mate with record A on contig u and read length L adds 1 to disc[j] over the stretch in which its partner
 * should have been found: orient 0, s = A.cstart - A.rstart, [max(s, 0), min(s + max_insert, len_u)); orient 1,
 * e = A.cstop + (L - A.rstop), [max(e - max_insert, 0), min(e, len_u)); iff the interval is not empty.  Separators hold 0 in
 * both tracks; counts are exact in 32 bits.
 *
 * Column i of contig u is WEAK iff margin <= i < len_u - margin, span <= max_span and disc >= min_disc; a contig of
 * 2 * margin bases or fewer has no weak column.  A RUN [a, b) is a maximal stretch of consecutive weak columns of one
 * contig; it is a BREAK iff b - a >= min_run, and the contig is then cut at m = a + (b - a) / 2 into [.., m) and [m, ..).
 * Because margin >= 1 every piece is non-empty.  margin >= max_insert keeps a contig's own ends from looking like joins: a
 * fragment that starts at least max_insert inside a contig ends inside it, so its mate lies on that contig; nearer an end
 * the mate may honestly lie beyond it, on another contig or nowhere, and such mates are discordant without any misjoin.
 *
 * Output.  seqs_out is the input block with one '_' inserted in front of column m of every break: n_ctgs + breaks contigs in
 * nbytes + breaks bytes, a block kc_ctg_index_build, kc_submit_ctg_block, kc_ctg_dedup, kc_ctg_select and kc_fasta_text take
 * as it is.  offsets_out (may be NULL): *n_out + 1 starts.  depths_out (written only if depths was given; may be NULL):
 * gathered the same way, 0 on every separator.  pieces (may be NULL): one record per output contig in block order; flags
 * bit 0 is set iff the piece begins at a cut, bit 1 iff it ends at one.  breaks (may be NULL): one record per break,
 * ascending in block position; pos, run_start in contig coordinates; more than break_capacity of them is KC_ERR_CAPACITY,
 * never a truncation.  span_out, disc_out (each may be NULL): uint16_t[nbytes] over the INPUT block, min(v, 65535).  Every
 * output is one exact byte string, independent of the order of the records.
 * Room: seqs_out and depths_out hold `capacity` elements; with x = capacity - nbytes, offsets_out holds n_ctgs + x + 1
 * entries and pieces n_ctgs + x records (a block that fits has at most x breaks).
 *
 * Statistics: pairs = spanning + discordant_pairs + one_mate + none; disc_mates the discordant mates whose interval
 * contributed; empty_intervals the spanning pairs' and discordant mates' intervals that were empty; columns = nbytes - n_ctgs;
 * interior the columns with margin <= i < len_u - margin; weak; runs = short_runs + breaks; broken_contigs;
 * pieces = n_ctgs + breaks; span_sum, disc_sum the tracks' exact sums.
 *
 * The protocol is kc_ctg_dedup's.  KC_ERR_INVALID_ARG before the context, kc_last_error naming the value: NULL params, n_out
 * or nbytes_out; unknown flags; non-zero reserved words; max_insert outside 1 .. KC_INSERT_MAX; margin 0; min_run 0; odd
 * nreads.  Then KC_ERR_INVALID_ARG for a NULL ctx, NULL offsets, alns or pairs with non-zero counts, misaligned device arrays
 * (records 16 bytes, offsets 8, uint16 arrays 2).  KC_ERR_STATE without an index.  KC_ERR_CAPACITY for 2^32 records or reads
 * or more.  From the device checks, before anything is stored, KC_ERR_INVALID_ARG with the lowest bad index named: a read
 * over KC_ALIGN_MAX_READ_LEN or with decreasing offsets, then an invalid record, then an invalid pair.  seqs_out == NULL is a
 * size query: *n_out, *nbytes_out and *stats are written and nothing else.  capacity < *nbytes_out: KC_ERR_CAPACITY with the
 * same three written.  One break more than break_capacity (with breaks != NULL): KC_ERR_CAPACITY.  n_alns == 0, or no break at
 * all, is KC_OK with the block copied unchanged.  On every other error nothing is written through any pointer.  The index,
 * the table and the results are untouched; the call runs on the context's stream, works with rank_n > 1, keeps no state and
 * frees its scratch: 9 bytes a block byte (two 32-bit tracks and a weak flag, scanned in tiles of T = 2048 columns with 32
 * bytes a tile), 16 bytes a break, and the copies of a host caller's arrays.  on_device != 0: every array but params, n_out,
 * nbytes_out and stats is a device pointer.
 */
#define KC_BREAK_ONE_MATE 1u
typedef struct kc_break_params { /* 32 bytes */
  uint32_t max_insert;   /* 1 .. KC_INSERT_MAX */
  uint32_t max_span;     /* a column with more spanning pairs is never weak */
  uint32_t min_disc;     /* a column with fewer discordant mates is never weak; 0 allowed */
  uint32_t margin;       /* >= 1: columns nearer than this to either contig end are never weak */
  uint32_t min_run;      /* >= 1: a weak run shorter than this is no break */
  uint32_t flags;        /* KC_BREAK_ONE_MATE */
  uint32_t reserved[2];  /* zero */
} kc_break_params;
typedef struct kc_break_piece { /* 16 bytes, one per output contig */
  uint32_t ctg;          /* the input contig */
  uint32_t start, len;   /* the piece is its columns [start, start + len) */
  uint32_t flags;        /* bit 0: begins at a cut; bit 1: ends at one */
} kc_break_piece;
typedef struct kc_break_rec { /* 32 bytes, one per break */
  uint32_t ctg;
  uint32_t pos;          /* m, in the contig */
  uint32_t run_start, run_len; /* a, b - a */
  uint32_t span, disc;   /* the exact counts at m */
  uint32_t piece;        /* the index of the piece that begins at m */
  uint32_t pad;          /* zero */
} kc_break_rec;
typedef struct kc_break_stats { /* 128 bytes */
  uint64_t pairs, spanning, discordant_pairs, one_mate, none;
  uint64_t disc_mates, empty_intervals;
  uint64_t span_sum, disc_sum;
  uint32_t columns, interior, weak;
  uint32_t runs, short_runs, breaks;
  uint32_t broken_contigs, pieces;
  uint32_t reserved[6];  /* zero */
} kc_break_stats;
int kc_ctg_break(kc_ctx *ctx, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns,
                 const kc_pair_rec *pairs, const uint16_t *depths, int on_device, const kc_break_params *params,
                 uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out, uint16_t *depths_out, kc_break_piece *pieces,
                 kc_break_rec *breaks, uint64_t break_capacity, uint16_t *span_out, uint16_t *disc_out, uint64_t *n_out,
                 uint64_t *nbytes_out, kc_break_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
