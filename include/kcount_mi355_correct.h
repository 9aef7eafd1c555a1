/* kcount_mi355_correct.h -- the second public header of libkcount_mi355.so: read correction from the finished k-mer table
 * (tests/correct_model.py).  It includes kcount_mi355.h and adds one entry point.  The entry point has a
 * header of its own because tests/test_abi.py and tests/test_entry_point_coverage_all.py hold the first header to closed
 * lists; tests/test_entry_point_coverage_correct.py holds this one to the same rule.
 */
#ifndef KCOUNT_MI355_CORRECT_H
#define KCOUNT_MI355_CORRECT_H

#include "kcount_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kc_correct_reads: substitutions from the k-mer spectrum ---------------------------------------------------------------
 * The reference holds no read correction (it relies on dmin_thres and the extension vote), so the rules are this project's own.
 *
 * Input as kc_seq_kmer_depths takes it: sequence i is bytes [offsets[i], offsets[i+1]) of bases; offsets[0] = 0,
 * offsets[nseqs] = nbytes, offsets never decrease, empty sequences are allowed.  quals (may be NULL) has nbytes bytes beside
 * the bases and is only read when max_qual > 0.  out has nbytes bytes, does not overlap bases, and shares the offsets: every
 * byte that is not corrected is copied unchanged, and lengths never change (substitutions only; an N is never turned into a
 * base; qualities are not rewritten).
 *
 * Definitions (those of kc_seq_kmer_depths).  Position p of sequence i is a window iff p + k <= offsets[i+1] and all k bytes
 * are A C G T a c g t.  Its count is that of its canonical upper-cased k-mer among the results, 0 when absent.  With
 * S = max(min_count, 1) a window is solid iff its count >= S, weak otherwise; a non-window is neither.  A weak run is a maximal
 * [a, b] of consecutive positions of one sequence that are all weak windows, L = b - a + 1; it is left-anchored iff a - 1 is a
 * solid window of the same sequence and right-anchored iff b + 1 is.
 *
 * One round is a pure function of the current text and the table.  The left site of a left-anchored run is byte
 * e = a + k - 1 with the range of windows a, a+1, .., min(a + k - 1, b), ascending; the right site of a right-anchored run is
 * byte e = b with the range b, b-1, .., max(b - k + 1, a), descending.  n = min(k, L) is the range's length and every window of
 * it holds e.  A run without an anchor gives no site (KC_CORRECT_UNANCHORED); one anchor gives that side's site; two anchors
 * give none when L < k (KC_CORRECT_SHORT_RUN: not what one substitution leaves), the left site when k <= L < 2k (the right one
 * follows in a later round) and both when L >= 2k.  A site with n < min_windows is dropped (KC_CORRECT_THIN); else, with quals
 * given and max_qual > 0, a site with quals[e] - qual_offset > max_qual is dropped (KC_CORRECT_QUAL_GATED).  For each of the
 * three bases y other than the one at e, score(y) is the number of leading windows of the range, in its order, that are solid
 * with byte e read as y.  The site is accepted for y* iff score(y*) >= min(n, min_gain) and score(y*) is greater than both
 * other scores; all scores below that need is KC_CORRECT_NO_GAIN, a best score that meets it and is tied is
 * KC_CORRECT_AMBIGUOUS.  An accepted site writes "ACGT"[y*] | (old & 0x20).  All sites of a round are evaluated before any is
 * applied; no window of one evaluated site holds another, so the order does not matter.  Round r + 1 runs on round r's output;
 * the call stops after `rounds` rounds or after the first round that accepts nothing.
 *
 * recs (one per sequence, may be NULL): weak windows of the input and of out, the number of corrected bytes (saturating), and
 * the OR of the reasons of the runs and sites left in the last evaluated round.  fixes (may be NULL): one entry per corrected
 * byte, ordered by (round, seq, pos); more than fix_capacity of them is KC_ERR_CAPACITY with no caller array touched, never a
 * truncation; fixes == NULL needs no capacity.  stats (may be NULL) is the host's.
 *
 * KC_ERR_INVALID_ARG, before any device call: NULL ctx / params / offsets, NULL bases or out with nbytes > 0, min_count > 65535,
 * min_gain == 0, rounds outside 1 .. 8, max_qual > 255, non-zero flags or reserved words, misaligned device arrays (offsets 8
 * bytes, recs and fixes 16); rank_n > 1 (a k-mer of another rank looks absent; correcting against a shard is wrong); from the
 * device check, before anything is stored: offsets that go backwards, offsets[0] != 0, offsets[nseqs] != nbytes.
 * KC_ERR_CAPACITY: 2^32 sequences or more, a sequence of 2^32 bytes or more, too many fixes.  KC_ERR_STATE before kc_finalize.
 * nseqs == 0 or nbytes == 0: KC_OK without a look at the offsets, zeroed recs and stats, out = bases.  The call uses the
 * lookup index of kc_lookup and builds it if absent; the results are not sorted, moved or touched.  It runs on the context's
 * stream and returns when its work there is done; its scratch (3 bytes a text byte, 20 bytes a sequence, 48 bytes a site of a
 * round, the copies of host arrays) lives for the call.  on_device != 0: bases, quals, offsets, out, recs and fixes are device
 * pointers.
 */
#define KC_CORRECT_UNANCHORED 1u
#define KC_CORRECT_SHORT_RUN 2u
#define KC_CORRECT_THIN 4u
#define KC_CORRECT_QUAL_GATED 8u
#define KC_CORRECT_NO_GAIN 16u
#define KC_CORRECT_AMBIGUOUS 32u
#define KC_CORRECT_MAX_ROUNDS 8
#define KC_CORRECT_LEFT 0
#define KC_CORRECT_RIGHT 1
typedef struct kc_correct_params { /* 32 bytes */
  uint32_t min_count;               /* a window is solid when its count >= max(min_count, 1); at most 65535 */
  uint32_t min_gain;                /* a site needs min(n, min_gain) leading solid windows; at least 1 */
  uint32_t min_windows;             /* a site with a shorter range is dropped */
  uint32_t rounds;                  /* 1 .. KC_CORRECT_MAX_ROUNDS */
  uint32_t max_qual;                /* 0: no gate; else only bytes with quals[e] - qual_offset <= max_qual are sites */
  uint32_t flags;                   /* zero */
  uint32_t reserved[2];             /* zero */
} kc_correct_params;
typedef struct kc_correct_rec { /* 16 bytes, one per sequence */
  uint32_t weak_before;          /* weak windows of the input */
  uint32_t weak_after;           /* weak windows of out */
  uint16_t corrected;            /* bytes changed, at most 65535 */
  uint16_t flags;                /* KC_CORRECT_* of the last evaluated round */
  uint32_t reserved;             /* zero */
} kc_correct_rec;
typedef struct kc_correct_fix { /* 16 bytes */
  uint32_t seq, pos;             /* pos within the sequence */
  uint8_t old_base, new_base;    /* the bytes */
  uint8_t round;                 /* from 1 */
  uint8_t side;                  /* KC_CORRECT_LEFT, KC_CORRECT_RIGHT */
  uint16_t score, runner_up;     /* the winner's score and the greater of the other two */
} kc_correct_fix;
typedef struct kc_correct_stats { /* 64 bytes */
  uint64_t seqs, bytes, windows;
  uint64_t weak_before, weak_after;
  uint64_t sites;                /* sites evaluated, over all rounds */
  uint64_t accepted;             /* = fixes */
  uint64_t rounds;               /* rounds run, with the one that accepted nothing */
} kc_correct_stats;
int kc_correct_reads(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets, uint64_t nseqs,
                     int on_device, const kc_correct_params *params, uint8_t *out, kc_correct_rec *recs, kc_correct_fix *fixes,
                     uint64_t fix_capacity, kc_correct_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
